"""What tests/test_sampler_walk_gpu.py relies on, checked without a GPU: the step-by-step reference of the nested chains
(tests/tools/sampler_walk.py) equals the unextended numpy restatements; on every case of the table the chains whose
decisions lie within the margins (the ones the GPU test leaves out) plus the chains whose walk changes when y is
shifted by +- the margin stay within the caps; the arithmetic noise floor of the reference (float64 against long double)
is below the EPS0 the position tolerance is made from, and that tolerance is far below the narrowest W; the tables cover
every (DP bucket, kernel id) instantiation, odd and even d in every bucket and both sides of every nsplit boundary."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import ns_philox  # noqa: E402
import sampler_walk as sw  # noqa: E402
from ns_cluster import ClusteredNumpyDevice  # noqa: E402
from ns_volumes import VolumesNumpyDevice  # noqa: E402

R, K = sw.R_STEPS, sw.N_CHAINS


@pytest.fixture(scope="module")
def table():
    """Per case: the generation, its trace, the traces with y shifted by +- Y_MARGIN and the long double trace."""
    out = {}
    for name in sw.NESTED_CASES:
        g = sw.Generation(name, gpr_device=OracleDevice())
        out[name] = dict(g=g, tr=g.trace(), up=g.trace(shift=sw.Y_MARGIN), down=g.trace(shift=-sw.Y_MARGIN),
                         ld=g.trace(dtype=np.longdouble))
    return out


def _left_out(e):
    """Chains the margins leave out by the last step, and chains whose walk differs under the shift of y."""
    tr = e["tr"]
    out = ~tr.keep(R)
    changed = np.zeros(K, bool)
    for other in (e["up"], e["down"]):
        changed |= np.any(other.U != tr.U, axis=(0, 2)) | np.any(other.ncalls != tr.ncalls, axis=0)
    return out, changed


@pytest.mark.parametrize("name", list(sw.NESTED_CASES))
def test_left_out_share_of_a_case(table, name):
    out, changed = _left_out(table[name])
    n = int(np.sum(out | changed))
    print(f"{name}: {int(out.sum())} of {K} chains within the margins, {int(changed.sum())} changed by the shift of y")
    assert n <= sw.LEFT_OUT_CASE * K, (name, n)
    # a walk that changes under the shift is one the margins leave out: what the GPU test compares is what is stable
    assert not np.any(changed & ~out), (name, np.flatnonzero(changed & ~out))


def test_left_out_share_of_the_table(table):
    n = sum(int(np.sum(np.logical_or(*_left_out(e)))) for e in table.values())
    assert n <= sw.LEFT_OUT_TABLE * K * len(table), n


def test_noise_floor_and_position_tolerance(table):
    eps, min_diag = 0.0, np.inf
    for name, e in table.items():
        tr, ld = e["tr"], e["ld"]
        for r in range(R + 1):
            both = tr.keep(r) & ld.keep(r)
            # the same decisions in both precisions for the chains the margins keep
            np.testing.assert_array_equal(tr.ncalls[r][both], ld.ncalls[r][both], err_msg=name)
            eps = max(eps, float(np.max(np.abs(tr.U[r][both] - ld.U[r][both]), initial=0.0)))
        min_diag = min(min_diag, e["g"].min_diag())
    print(f"eps0 = {eps:.3g} (EPS0 = {sw.EPS0:g}); smallest W diagonal = {min_diag:.3g}")
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:      # (where long double is wider than double)
        assert 0.0 < eps <= sw.EPS0, eps
    assert sw.POS_TOL == 100 * sw.EPS0 and sw.G_MARGIN == 100 * sw.EPS0 and sw.Y_MARGIN == 1e-9
    assert sw.POS_TOL < 1e-6 * min_diag, (sw.POS_TOL, min_diag)


def test_the_cases_are_the_degenerate_walks_they_claim(table):
    tr = table["W narrow (1e-3)"]["tr"]
    assert np.sum(tr.stepout == ns_philox.STEP_OUT_MAX) > 0
    # after the cap of 32 widths the walk goes on to shrink: the capped chains moved all the same
    capped = tr.stepout == ns_philox.STEP_OUT_MAX
    assert np.all(np.any(tr.U[R][capped] != tr.U[0][capped], axis=1))
    wide = table["W wide (50)"]["tr"]
    assert np.mean(wide.ncalls[R]) < 0.5 * np.mean(table["d=3 kid=3 N=600 affine=on"]["tr"].ncalls[R])
    for name in ("plateau", "every try gated"):
        t = table[name]["tr"]
        np.testing.assert_array_equal(t.U[R], t.U[0])
        np.testing.assert_array_equal(t.y[R], t.y[0])
        full = R * (2 + ns_philox.SHRINK_MAX)
        assert np.all(t.ncalls[R] <= full) and np.all(t.ncalls[R] > full - 3 * R * 4)
    assert np.any(table["plateau"]["tr"].ncalls[R] < R * (2 + ns_philox.SHRINK_MAX)), "no try left the box"
    assert np.all(table["plateau"]["tr"].y == table["plateau"]["g"].clip_hi)
    gt = table["every try gated"]["tr"]
    np.testing.assert_array_equal(gt.gated, gt.ncalls[R])
    assert np.sum(table["SVM + trust region"]["tr"].gated) > 0
    f = table["starts on the faces"]
    U0 = f["tr"].U[0]
    assert np.sum((U0 == 0.0) | (U0 == 1.0)) >= 2, "no chain starts on a face"
    v = table["volumes"]
    assert set(v["tr"].cluster) == {0, 2, 3} and np.sum(v["g"].labels == 3) == 1
    assert set(table["clustered"]["tr"].cluster) == {0, 1, 2}


def test_the_tables_cover_every_instantiation_and_every_edge():
    pairs = lambda rows: {(sw.dp_bucket(d), kid) for d, kid in rows}          # noqa: E731
    every = {(dp, kid) for dp in (4, 8, 16, 32) for kid in range(4)}
    plain = [(d, kid) for d, kid, N, aff in sw.PLAIN_ROWS]
    assert pairs(plain) == every
    assert pairs((d, kid) for N, d, kid, aff in sw.EVAL_CASES) == every
    for rows in ([d for d, kid in plain], [d for N, d, kid, aff in sw.EVAL_CASES]):
        for dp in (4, 8, 16, 32):
            in_bucket = [d for d in rows if sw.dp_bucket(d) == dp]
            assert any(d % 2 for d in in_bucket) and any(d % 2 == 0 for d in in_bucket), dp
        assert {1, 32} <= set(rows)
    assert {d for d, kid in plain} == {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32}
    assert {N for d, kid, N, aff in sw.PLAIN_ROWS} == {17, 600, 2048, 4096}
    assert {aff for d, kid, N, aff in sw.PLAIN_ROWS} == {True, False}
    variants = {v for m, v in sw.NESTED_CASES.values()}
    assert variants == {"plain", "narrow", "wide", "plateau", "clustered", "volumes", "faces", "gated"}
    assert {"clip active", "SVM + trust region"} <= set(sw.NESTED_CASES)
    Ns = sorted({N for N, d, kid, aff in sw.EVAL_CASES})
    assert set(Ns) >= {1, 2, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 9217}
    # both sides of every change of nsplit below the clamp, both sides of a multiple of 32 at one slice, and the clamp
    for edge in (2048, 8192):
        assert edge - 1 in Ns and edge in Ns and sw.nsplit(edge - 1) != sw.nsplit(edge)
    assert 31 in Ns and 32 in Ns and 33 in Ns and max(Ns) > 9216 and sw.nsplit(max(Ns)) == 8
    assert {aff for N, d, kid, aff in sw.EVAL_CASES} == {True, False}


@pytest.mark.parametrize("name", ["d=3 kid=3 N=600 affine=on", "d=17 kid=2 N=600 affine=on", "W narrow (1e-3)",
                                  "clip active", "clustered", "volumes", "starts on the faces"])
def test_the_trace_ends_where_the_unextended_restatement_ends(table, name):
    g, tr = table[name]["g"], table[name]["tr"]
    ll = lambda X: np.minimum(g.mean(X), g.clip_hi)          # noqa: E731
    kind = VolumesNumpyDevice if g.cum_p is not None else ClusteredNumpyDevice if g.labels is not None \
        else ns_philox.NumpyNestedDevice
    for r in (0, 1, R):
        X, y, cnt, _ = g.device_call(kind(ll), r)
        np.testing.assert_array_equal(X, tr.X[r])
        np.testing.assert_array_equal(y, tr.y[r])
        np.testing.assert_array_equal(cnt, tr.ncalls[r])


def test_only_the_lower_triangle_of_W_is_read():
    g = sw.Generation("d=3 kid=3 N=600 affine=on", gpr_device=OracleDevice())
    ll = lambda X: np.minimum(g.mean(X), g.clip_hi)          # noqa: E731
    a = g.device_call(ns_philox.NumpyNestedDevice(ll), 3)
    g.W = g.W + np.triu(np.full_like(g.W, 0.7), 1)
    b = g.device_call(ns_philox.NumpyNestedDevice(ll), 3)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(g.trace(R=3).X[3], a[0])


def test_the_mirror_on_the_oracle_device_agrees_with_the_reference_likelihood():
    """The reference's likelihood (oracle mean, host-side masks) is what the mirror class computes."""
    for name in ("SVM + trust region", "clip active", "d=2 kid=1 N=600 affine=off"):
        g = sw.Generation(name, gpr_device=OracleDevice())
        gpr = g.gpr if g.gpr is not None else g.model.gpr(device=OracleDevice())
        X = ns_philox.prior_points(g.lo, g.hi, 5, 200)
        ref = np.minimum(g.mean(X), g.clip_hi)
        got = gpr.predict(X)
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
        fin = np.isfinite(ref)
        assert np.max(np.abs(got[fin] - ref[fin])) <= g.model.tol()


@pytest.mark.parametrize("thin,given,miv", [(1, False, -np.inf), (3, True, -np.inf), (3, False, -3.0)])
def test_the_metropolis_rule_check_accepts_the_numpy_stand_in_and_refuses_a_wrong_one(thin, given, miv):
    """The check the GPU file runs on the kernel, run on the numpy stand-in of the same algorithm -- and on one whose
    acceptance uniform is another draw, which it must refuse."""
    import mcmc_numpy
    d, n = 5, 16
    ll = sw.gauss_ll(d)
    lo, hi = np.full(d, -4.0), np.full(d, 4.0)
    X0 = np.random.default_rng(1).normal(0.3, 0.5, (n, d))
    y_true = ll(X0)
    y0, y_start = (y_true - 0.25, y_true - 0.25) if given else (np.full(n, np.nan), y_true)
    Lp = 0.04 * np.tril(np.ones((d, d)))
    args = (lo, hi, X0, y0, y_start, Lp, 1.5, miv, 99, 2, 40, thin)
    counts = sw.check_metropolis_rule(mcmc_numpy.NumpyMCMCDevice(ll), *args, oracle_y=ll, oracle_tol=1e-12)
    assert counts["accepted"] > 0 and counts["borderline"] == 0
    if np.isfinite(miv):
        assert counts["below_minus_inf_value"] > 0

    class Wrong(mcmc_numpy.NumpyMCMCDevice):
        def mcmc_chains(self, *a, **kw):
            keep = mcmc_numpy.DRAW_ACCEPT
            mcmc_numpy.DRAW_ACCEPT = 15
            try:
                return super().mcmc_chains(*a, **kw)
            finally:
                mcmc_numpy.DRAW_ACCEPT = keep

    with pytest.raises(AssertionError):
        sw.check_metropolis_rule(Wrong(ll), *args)
