"""``gpry_predict_without`` on the device: the change of mean and variance at M points when a group of training points is
taken out, against the numpy truth (tests/tools/predict_without_model.py), the exact facts, the family (``loo``,
``leave_out``), the bits contract, the state contract, the refusals, a grown factor and ``batch_influence`` end to end.

Models: ``pm.CASES`` (tests/test_predict_thetas_gpu.py says what each shape exercises).  Points: ``tm.points``, 26 -- 8
training rows (0 and 1, duplicates, among them), 16 uniform, 2 far outside where k* underflows -- and, for the family
checks, the last 16 training rows behind them.  Groups: ``wm.groups_of`` -- {0} (its duplicate stays in), {N - 1}, five
unsorted indices with 0 and N - 1, the last 16 rows (a full padding tile), 17 (crosses it), 64 random (48 at N = 50), two
overlapping groups, and the last 16 once more.

The bound, per group, for dmean and dvar separately: max_i |dev - a| <= max(10 max_i |a - b|, 2 D_seq), a / b the two numpy
formulations (refit without the rows / downdate from the full factor) and D_seq the deviation from (a) of the route that
exists without this call, on a second context in the same test: the model loaded without the rows at the same theta,
factorize, unclipped predict with std, minus the full model's -- the rule of test_predict_thetas_gpu.py /
test_predict_thetas_var_gpu.py.

Internal sizes the bit tests cross (predict_without.hip): a batch of groups holds 1024 stacked rows, a group padded to a
multiple of 16 (65 singletons cross it); a panel 2048 points; an upload 32768 points.

Measured on an MI355X (worst deviation / bound over the groups and both quantities of a case; profiles/predict_without.md):
n50_d1_k1 0.168; n130_d2 k0 0.298, k0_w 0.139, k1 0.221, k1_w 0.425, k2 0.327, k2_w 0.257, k3 0.600, k3_w 0.226; n333_d5_k2_w
0.118; n300_d17_k2_w 0.100; n256_d32_k0 0.496; n1100_d8_k3_w 0.147; n2500_d4_k1 0.413.  The family checks (loo, leave_out) use
at most 0.494 of the bound, the grown factors 0.178; end to end |dlogZ - numpy| = 7.6e-15 and |kl - numpy| = 2.2e-16 against a
bound on dmean of 4.8e-13.
"""
import ctypes as C
import math
import os
import sys
import warnings

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict_thetas_model as pm  # noqa: E402
import predict_without_model as wm  # noqa: E402
import theta_grad_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def other():
    from gpry_amd import _lib
    d = _lib.Device(0)
    yield d
    d.close()


def flag(case):
    return case[2] | tm.W_FLAG if case[3] else case[2]


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a if k != "device_ms")
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def pw(dev, groups, Xq):
    out = dev.predict_without(groups, Xq)
    return np.stack([out["dmean"], out["dvar"]])                # (2, ngroups, M)


_ref = {}


def reference(case):
    """(X_, y_, alpha, theta, groups, Xq_ (42 unit points), A (2, ngroups, 42), B likewise): computed once, never changed."""
    if case not in _ref:
        N, d, kid, white = case
        X_, y_, a, th = tm.problem(N, d, seed=N + d, white=white)
        Xq_ = np.concatenate([tm.points(case, X_), X_[N - 16:]])
        groups = [g for _, g in wm.groups_of(N)]
        K, _ = tm._matrices(X_, a, th, kid, white)
        V = solve_triangular(cholesky(K, lower=True), np.eye(N), lower=True)
        al = V.T.dot(V.dot(y_))
        ks = wm._cross(X_, th, kid, Xq_)
        A = np.stack([np.stack(wm.refit_K(K, y_, ks, g, tm.Y_STD)) for g in groups], axis=1)
        B = np.stack([np.stack(wm.downdate_V(V, al, ks, g, tm.Y_STD)) for g in groups], axis=1)
        for arr in (Xq_, A, B):
            arr.setflags(write=False)
        _ref[case] = (X_, y_, a, th, groups, Xq_, A, B)
    return _ref[case]


def sequential(other, case, X_, y_, a, th, g, Xq, full):
    """The route without the call: the model without the rows on ``other``, factorised, predict with std, minus the full
    model's (mean, std^2)."""
    keep = np.setdiff1d(np.arange(len(y_)), g)
    lo, span = tm.affine(case)
    other.set_train(X_[keep], y_[keep], a[keep])
    other.set_theta(flag(case), th)
    other.set_affine(lo, span, tm.Y_MEAN, tm.Y_STD, np.inf)
    assert other.factorize() == 0
    m, s = other.predict(Xq, return_std=True)
    return np.stack([m - full[0], s * s - full[1] * full[1]])


# ------------------------------------------------------------------------------------ against the closed form, the family
@pytest.mark.parametrize("case", pm.CASES, ids=pm.IDS)
def test_against_the_closed_form_the_exact_facts_and_the_family(dev, other, case):
    N, d, kid, white = case
    name = pm.IDS[pm.CASES.index(case)]
    X_, y_, a, th, groups, Xq_, A, B = reference(case)
    tm.load(dev, case)
    Xq = tm.to_raw(case, Xq_)
    out = dev.predict_without(groups, Xq)
    got = np.stack([out["dmean"], out["dvar"]])
    assert got.shape == (2, len(groups), 42) and np.isfinite(got).all() and out["device_ms"] > 0
    assert not out["info"].any()
    assert np.all(out["dvar"] >= 0.0)
    assert np.all(out["dmean"][:, 24:26] == 0.0) and np.all(out["dvar"][:, 24:26] == 0.0)       # k* underflows: exactly nothing
    full = dev.predict(Xq, return_std=True)                     # (the case is loaded without a clip and without gates)
    loo = dev.loo()
    worst = 0.0
    bounds = np.empty((2, len(groups), 2))                      # [quantity, group, (the 26 points, the 16 training rows)]
    for k, g in enumerate(groups):
        seq = sequential(other, case, X_, y_, a, th, g, Xq, full)
        for q, what in enumerate(("dmean", "dvar")):
            for part, sl in enumerate((slice(0, 26), slice(26, 42))):
                ab = np.max(np.abs(A[q, k, sl] - B[q, k, sl]))
                d_seq = np.max(np.abs(seq[q, sl] - A[q, k, sl]))
                bounds[q, k, part] = max(10.0 * ab, 2.0 * d_seq)
            ab = np.max(np.abs(A[q, k, :26] - B[q, k, :26]))
            d_seq = np.max(np.abs(seq[q, :26] - A[q, k, :26]))
            d_dev = np.max(np.abs(got[q, k, :26] - A[q, k, :26]))
            bound = bounds[q, k, 0]
            print(f"predict_without {name} group {k} (n = {len(g)}) {what}: deviation {d_dev:.3e} at size {np.max(np.abs(A[q, k, :26])):.3e}, "
                  f"a-b {ab:.3e}, sequential route {d_seq:.3e}, ratio {d_dev / bound:.3f}")
            worst = max(worst, d_dev / bound)
            assert d_dev <= bound, (k, what, d_dev, ab, d_seq)
    print(f"predict_without {name}: worst ratio {worst:.3f}")
    # the group listed twice; the overlap changes neither group
    assert np.array_equal(got[:, 3], got[:, 8])
    # a singleton at its own training row is leave-one-out: Xq[0] is training row 0, Xq[41] is row N - 1
    # (predict's std^2 of a model with a white term carries w, the latent variance does not)
    w_ys2 = tm.Y_STD * tm.Y_STD * math.exp(th[d + 1]) if white else 0.0
    for k, col, i in ((0, 0, 0), (1, 41, N - 1)):
        part = 0 if col < 26 else 1
        dm = abs(full[0][col] + out["dmean"][k, col] - loo["mean"][i])
        dv = abs((full[1][col] ** 2 - w_ys2) + out["dvar"][k, col] - loo["var_f"][i])
        print(f"predict_without {name} singleton {i} against loo: mean {dm:.3e} / {bounds[0, k, part]:.3e}, var_f {dv:.3e} / {bounds[1, k, part]:.3e}")
        assert dm <= bounds[0, k, part] and dv <= bounds[1, k, part], (i, dm, dv, bounds[:, k, part])
    # the last 16 rows at their own rows: the joint mean of leave_out
    lgo = dev.leave_out([groups[3]])
    dj = np.max(np.abs(full[0][26:] + out["dmean"][3, 26:] - lgo["mean"][0]))
    print(f"predict_without {name} last 16 against leave_out: {dj:.3e} / {bounds[0, 3, 1]:.3e}")
    assert dj <= bounds[0, 3, 1]


# ------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("case", [(130, 2, 2, True), (1100, 8, 3, True)])
def test_same_bits_whatever_the_points_the_groups_their_order_the_split_and_the_context(dev, other, case):
    X_, y_, a, th, groups, Xq_, A, B = reference(case)
    tm.load(dev, case)
    Xq = tm.to_raw(case, Xq_[:26])
    whole = pw(dev, groups, Xq)
    assert np.array_equal(pw(dev, groups, Xq), whole)                               # a second call repeats the first
    # a point alone, at another position, in split calls
    for i in (0, 9, 25):
        assert np.array_equal(pw(dev, groups, Xq[i:i + 1])[:, :, 0], whole[:, :, i]), i
    pp = np.random.default_rng(1).permutation(len(Xq))
    assert np.array_equal(pw(dev, groups, Xq[pp]), whole[:, :, pp])
    assert np.array_equal(np.concatenate([pw(dev, groups, Xq[:11]), pw(dev, groups, Xq[11:])], axis=2), whole)
    # a group alone, among others, at another position, its indices permuted; one output alone
    for k in range(len(groups)):
        assert np.array_equal(pw(dev, [groups[k]], Xq)[:, 0], whole[:, k]), k
    rev = list(range(len(groups)))[::-1]
    assert np.array_equal(pw(dev, [groups[k] for k in rev], Xq), whole[:, rev])
    rng = np.random.default_rng(2)
    assert np.array_equal(pw(dev, [rng.permutation(g) for g in groups], Xq), whole)
    assert np.array_equal(np.concatenate([pw(dev, groups[:4], Xq), pw(dev, groups[4:], Xq)], axis=1), whole)
    only = dev.predict_without(groups, Xq, want=("dvar",))
    assert only["dmean"] is None and np.array_equal(only["dvar"], whole[1])
    only = dev.predict_without(groups, Xq, want=("dmean",))
    assert only["dvar"] is None and np.array_equal(only["dmean"], whole[0])
    # a second context
    tm.load(other, case)
    assert np.array_equal(pw(other, groups, Xq), whole)


def test_the_internal_batch_of_groups(dev):
    """70 singletons (16 stacked rows each: 64 fill a batch) and then the case's own groups: two batches, the second mixed."""
    case = (130, 2, 1, False)
    X_, y_, a, th, groups, Xq_, A, B = reference(case)
    tm.load(dev, case)
    Xq = tm.to_raw(case, Xq_[:26])
    many = [np.array([i]) for i in range(70)] + groups
    assert 16 * 70 > wm.GROUP_BATCH_ROWS
    dev.timing_reset()
    out = pw(dev, many, Xq)
    assert dev.timing("without_setup")[1] == 2 and dev.timing("without_points")[1] == 2
    assert np.array_equal(out[:, 70:], pw(dev, groups, Xq))
    for i in (0, 63, 64, 69):
        assert np.array_equal(out[:, i], pw(dev, [[i]], Xq)[:, 0]), i
    assert np.array_equal(out[:, 0], out[:, 70])                                   # {0} twice, in two batches


def test_the_panel_and_upload_boundaries_of_the_points(dev):
    case = (130, 2, 0, False)
    X_, y_, a, th, groups, Xq_, A, B = reference(case)
    tm.load(dev, case)
    Xq26 = tm.to_raw(case, Xq_[:26])
    M = wm.UPLOAD_POINTS + 5
    Xq = tm.to_raw(case, np.random.default_rng(5).uniform(0, 1, (M, 2)))
    P, U = wm.PANEL_POINTS, wm.UPLOAD_POINTS
    at = np.concatenate([np.arange(P - 5, P + 5), np.arange(U - 6, U + 5), np.arange(5)])      # across a panel, across an upload, the start
    assert len(at) == 26
    Xq[at] = Xq26
    gs = [groups[0], groups[4], groups[5]]
    dev.timing_reset()
    out = pw(dev, gs, Xq)
    assert dev.timing("without_setup")[1] == 1 and dev.timing("without_points")[1] == U // P + 1
    few = pw(dev, gs, Xq26)
    assert np.array_equal(out[:, :, at], few)
    assert np.all(out[1] >= 0.0) and np.isfinite(out).all()


# ------------------------------------------------------------------------------------ state
@pytest.mark.parametrize("case", [(50, 1, 1, False), (333, 5, 3, True), (1100, 8, 2, False)])
def test_no_other_entry_point_notices_the_call_and_the_call_notices_none_of_them(dev, other, case):
    N, d, kid, white = case
    X_, y_, a, th = tm.load(other, case)
    Xq = tm.to_raw(case, tm.points(case, X_))
    groups = [g for _, g in wm.groups_of(N)]
    fresh = other.predict_without(groups, Xq)
    tm.load(dev, case)
    alt = th.copy()
    alt[:d + 1] += 0.1
    rng = np.random.default_rng(N)
    pool = tm.to_raw(case, rng.uniform(0, 1, (1500, d)))
    kbx = tm.to_raw(case, rng.uniform(0, 1, (40, d)))
    dev.sweep_logexp(pool, 1.0, float(np.max(y_)) * tm.Y_STD + tm.Y_MEAN, 1e-2)
    dev.kb_reset()
    dev.kb_register(kbx)

    def loo():
        r = dev.loo()
        return [r[k] for k in ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")]
    ops = [("predict_std", lambda: dev.predict(Xq, return_std=True)), ("sweep_fetch", lambda: dev.sweep_fetch(("y", "sigma", "acq"))),
           ("kb_gram", lambda: dev.kb_gram(39, 40)), ("loo", loo), ("lml_cached", lambda: dev.lml(alt, True)),
           ("predict_1", lambda: dev.predict(Xq[:1])), ("leave_out", lambda: dev.leave_out(groups[:4]))]
    before = [f() for _, f in ops]
    assert same_bits(dev.predict_without(groups, Xq), fresh)
    after = [f() for _, f in ops]
    for (name, _), x, y in zip(ops, before, after):
        assert same_bits(x, y), name
    for name, f in ops:
        f()
        assert same_bits(dev.predict_without(groups, Xq), fresh), name
    # the factor cache of gpry_lml: a factor adopted after the call is the theta's own
    dev.lml(alt, True)
    dev.predict_without(groups, Xq)
    dev.set_theta(flag(case), alt)
    assert dev.factorize() == 0
    got = dev.predict(Xq, return_std=True)
    other.set_theta(flag(case), alt)
    assert other.factorize() == 0
    assert same_bits(got, other.predict(Xq, return_std=True))


def test_refusals_return_minus_one_with_a_message_and_the_context_answers_as_before(dev):
    from gpry_amd import _lib
    case = (130, 2, 1, True)
    X_, y_, a, th, groups, Xq_, A, B = reference(case)
    tm.load(dev, case)
    Xq = tm.to_raw(case, Xq_[:26])
    good = dev.predict(Xq, return_std=True)
    answer = dev.predict_without(groups, Xq)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)  # noqa: E731
    i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)  # noqa: E731
    X = np.ascontiguousarray(Xq[:2])
    idx, off = i64([0, 5, 7]), i64([0, 1, 3])
    dm, dv, info = np.empty((2, 2)), np.empty((2, 2)), np.zeros(2, dtype=np.int32)
    xinf, xnan = X.copy(), X.copy()
    xinf[1, 0], xnan[0, 1] = np.inf, np.nan
    big = i64(np.arange(65))
    table = [("NULL idx", (None, vp(off), 2, vp(X), 2, vp(dm), vp(dv)), "NULL"), ("NULL offsets", (vp(idx), None, 2, vp(X), 2, vp(dm), vp(dv)), "NULL"),
             ("NULL X", (vp(idx), vp(off), 2, None, 2, vp(dm), vp(dv)), "NULL"), ("no output", (vp(idx), vp(off), 2, vp(X), 2, None, None), "both NULL"),
             ("ngroups 0", (vp(idx), vp(off), 0, vp(X), 2, vp(dm), vp(dv)), "ngroups = 0"),
             ("M 0", (vp(idx), vp(off), 2, vp(X), 0, vp(dm), vp(dv)), "M = 0"), ("M < 0", (vp(idx), vp(off), 2, vp(X), -3, vp(dm), vp(dv)), "M = -3"),
             ("x inf", (vp(idx), vp(off), 2, vp(xinf), 2, vp(dm), vp(dv)), "not finite"), ("x nan", (vp(idx), vp(off), 2, vp(xnan), 2, vp(dm), vp(dv)), "not finite"),
             ("empty group", (vp(idx), vp(i64([0, 0, 3])), 2, vp(X), 2, vp(dm), vp(dv)), "empty"),
             ("65 indices", (vp(big), vp(i64([0, 65])), 1, vp(X), 2, vp(dm), vp(dv)), "at most 64"),
             ("out of range", (vp(i64([0, 5, 130])), vp(off), 2, vp(X), 2, vp(dm), vp(dv)), "outside"),
             ("negative", (vp(i64([-1, 5, 7])), vp(off), 2, vp(X), 2, vp(dm), vp(dv)), "outside"),
             ("twice", (vp(i64([0, 5, 5])), vp(off), 2, vp(X), 2, vp(dm), vp(dv)), "more than once")]
    for what, args, word in table:
        rc = dev._lib.gpry_predict_without(dev._h, *args, vp(info), None)
        msg = dev._lib.gpry_last_error(dev._h).decode()
        assert rc == -1 and word in msg and "gpry_predict_without" in msg, (what, rc, msg)
        assert same_bits(dev.predict(Xq, return_std=True), good), what
        assert same_bits(dev.predict_without(groups, Xq), answer), what
    # info and device_ms are optional, and either output
    assert dev._lib.gpry_predict_without(dev._h, vp(idx), vp(off), 2, vp(X), 2, vp(dm), None, None, None) == 0
    assert dev._lib.gpry_predict_without(dev._h, vp(idx), vp(off), 2, vp(X), 2, None, vp(dv), None, None) == 0
    want = dev.predict_without([[0], [5, 7]], X)
    assert np.array_equal(dm, want["dmean"]) and np.array_equal(dv, want["dvar"])
    with pytest.raises(ValueError):
        dev.predict_without(groups, Xq[:, :1])
    with pytest.raises(ValueError):
        dev.predict_without(groups, Xq, want=())
    # no training set; a training set that is not factorised
    fresh = _lib.Device(dev.device)
    try:
        rc = fresh._lib.gpry_predict_without(fresh._h, vp(idx), vp(off), 2, vp(X), 2, vp(dm), vp(dv), None, None)
        assert rc == -1 and "factor" in fresh._lib.gpry_last_error(fresh._h).decode()
        fresh.set_train(X_, y_, a)
        fresh.set_theta(flag(case), th)
        rc = fresh._lib.gpry_predict_without(fresh._h, vp(idx), vp(off), 2, vp(X), 2, vp(dm), vp(dv), None, None)
        assert rc == -1 and "factor" in fresh._lib.gpry_last_error(fresh._h).decode()
    finally:
        fresh.close()
    assert same_bits(dev.predict_without(groups, Xq), answer)


# ------------------------------------------------------------------------------------ a grown factor
@pytest.mark.parametrize("case", [(130, 2, 2, True), (333, 5, 0, False)])
def test_a_factor_grown_by_append_rows(dev, other, case):
    N, d, kid, white = case
    X_, y_, a, th = tm.load(dev, case)
    rng = np.random.default_rng(9 + N)
    Xn = rng.uniform(0, 1, (4, d))
    yn = np.sin(3 * Xn.sum(1))
    assert dev.append_rows(Xn, yn, np.full(4, 1e-4)) == 0
    Xa, ya, aa = np.vstack([X_, Xn]), np.append(y_, yn), np.full(N + 4, 1e-4)
    g = np.arange(N, N + 4)
    Xq_ = np.concatenate([tm.points(case, X_), Xn])
    Xq = tm.to_raw(case, Xq_)
    out = dev.predict_without([g], Xq)
    assert not out["info"].any()
    A = np.stack(wm.refit(Xa, ya, aa, th, kid, white, g, Xq_, tm.Y_STD))
    B = np.stack(wm.downdate(Xa, ya, aa, th, kid, white, g, Xq_, tm.Y_STD))
    full = dev.predict(Xq, return_std=True)
    seq = sequential(other, case, Xa, ya, aa, th, g, Xq, full)
    for q, what in enumerate(("dmean", "dvar")):
        bound = max(10.0 * np.max(np.abs(A[q] - B[q])), 2.0 * np.max(np.abs(seq[q] - A[q])))
        d_dev = np.max(np.abs(out[what][0] - A[q]))
        print(f"predict_without grown n{N}_d{d}_k{kid} {what}: deviation {d_dev:.3e}, ratio {d_dev / bound:.3f}")
        assert d_dev <= bound, (what, d_dev, bound)


# ------------------------------------------------------------------------------------ the regressor
def test_batch_influence_end_to_end_on_a_fitted_regressor(other):
    from gpry_amd import _lib
    from gpry_amd.gpr import GaussianProcessRegressor
    from gpry_amd.kernels import RBF, ConstantKernel as Ck, WhiteKernel
    from gpry_amd.mc import batch_influence
    from gpry_amd.preprocessing import Normalize_bounds, Normalize_y
    N, d = 60, 2
    b = np.array([[0.0, 1.0]] * d)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (N + 4, d))
    y = np.sin(6.0 * X.mean(1)) + 0.1 * rng.standard_normal(N + 4)
    kernel = Ck(1.0, [1e-3, 1e4]) * RBF([1.0] * d, [1e-3, 10.]) + WhiteKernel(1e-2, [1e-6, 1e1])
    gpr = GaussianProcessRegressor(kernel=kernel, bounds=b, n_restarts_optimizer=2, noise_level=1e-2,
                                   preprocessing_X=Normalize_bounds(b), preprocessing_y=Normalize_y(),
                                   account_for_inf=None, random_state=7)
    gpr.append_to_data(X[:N], y[:N], fit_gpr=True)
    gpr.append_to_data(X[N:], y[N:], fit_gpr=False)
    assert gpr.n_last_appended_finite == 4 and len(gpr.y_train) == N + 4
    Xs = rng.uniform(0, 1, (512, d))
    ys, ss = gpr.predict(Xs, return_std=True)
    w = rng.uniform(0.5, 1.5, 512)
    theta0 = gpr.kernel_.theta.copy()
    n0, l0 = gpr.n_eval, gpr.n_eval_loglike
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = batch_influence(gpr, Xs, ys, w)
    assert (gpr.n_eval, gpr.n_eval_loglike) == (n0 + 512, l0) and r.n_points == 512 and r.device_ms > 0
    print(r)
    # numpy: the refit without the four rows at today's theta and maps
    kid, th_full = gpr.kernel_.device_spec(d)
    th_full = np.asarray(th_full, dtype=float)
    x_lo, x_span, y_mean, y_std = gpr._affine_args()[:4]
    Xu = Xs if x_lo is None else (Xs - np.asarray(x_lo)) / np.asarray(x_span)
    X_, y_ = np.asarray(gpr.X_train_, dtype=float), np.asarray(gpr.y_train_, dtype=float)
    al = np.array(np.broadcast_to(np.asarray(gpr.alpha, dtype=float), (N + 4,)))
    g = np.arange(N, N + 4)
    ma, va = wm.refit(X_, y_, al, th_full, kid & ~tm.W_FLAG, True, g, Xu, y_std)
    mb, vb = wm.downdate(X_, y_, al, th_full, kid & ~tm.W_FLAG, True, g, Xu, y_std)
    # ... and the sequential route on two fresh contexts
    seqs = []
    for keep in (np.arange(N + 4), np.arange(N)):
        other.set_train(X_[keep], y_[keep], al[keep])
        other.set_theta(kid, th_full)
        other.set_affine(x_lo, x_span, y_mean, y_std, np.inf)
        assert other.factorize() == 0
        seqs.append(other.predict(Xs, return_std=True))
    bound = max(10.0 * np.max(np.abs(ma - mb)), 2.0 * np.max(np.abs(seqs[1][0] - seqs[0][0] - ma)))
    bound_v = max(10.0 * np.max(np.abs(va - vb)), 2.0 * np.max(np.abs(seqs[1][1] ** 2 - seqs[0][1] ** 2 - va)))
    wk = w / w.sum()
    dlogZ = math.log(np.sum(wk * np.exp(ma)))
    kl = dlogZ - wk.dot(ma)
    p = wk * np.exp(ma)
    p /= p.sum()
    ess = 1.0 / np.sum(p * p)
    print(f"batch_influence end to end: dlogZ {r.dlogZ[0]:.6e} / numpy {dlogZ:.6e}, kl {r.kl[0]:.6e} / {kl:.6e}, ess {r.ess[0]:.3f} / {ess:.3f}, "
          f"bound on dmean {bound:.3e}, |dlogZ - numpy| {abs(r.dlogZ[0] - dlogZ):.3e}, |kl - numpy| {abs(r.kl[0] - kl):.3e}")
    assert abs(r.dlogZ[0] - dlogZ) <= bound and abs(r.kl[0] - kl) <= 2.0 * bound and r.kl[0] >= -2.0 * bound
    # (d ess / d log r is at most 2 ess per unit of log r in every row)
    assert abs(r.ess[0] - ess) <= 4.0 * ess * bound + 1e-9 * ess
    assert abs(r.var_gain[0] - wk.dot(va)) <= bound_v                  # (a weighted mean of deviations of at most bound_v)
    np.testing.assert_array_equal(r.groups[0], g)
    # the jackknife: N + 4 groups, the most influential point first
    each = batch_influence(gpr, Xs, ys, w, groups="each")
    assert len(each.groups) == N + 4 and each.kl.shape == (N + 4,) and not each.info.any()
    K, _ = tm._matrices(X_, al, th_full, kid & ~tm.W_FLAG, True)
    V = solve_triangular(cholesky(K, lower=True), np.eye(N + 4), lower=True)
    alf = V.T.dot(V.dot(y_))
    ks = wm._cross(X_, th_full, kid & ~tm.W_FLAG, Xu)
    kls = np.empty(N + 4)
    for i in range(N + 4):
        m = wm.downdate_V(V, alf, ks, [i], y_std)[0]
        kls[i] = math.log(np.sum(wk * np.exp(m))) - wk.dot(m)
    print(f"batch_influence each: order[:5] {each.order[:5]}, numpy {np.argsort(-kls)[:5]}, kl max {kls.max():.3e}")
    assert each.order[0] == int(np.argmax(kls))
    # nothing of the fitted model moved
    after = gpr.predict(Xs, return_std=True)
    assert np.array_equal(after[0], ys) and np.array_equal(after[1], ss) and np.array_equal(gpr.kernel_.theta, theta0)
