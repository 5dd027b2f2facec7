"""The tail of the pruned NORA sweep behind stage A: the small-launch tile map of the one-pass contraction (option
"sweep_small_map"), the radix select without scan launches ("select_fused") and the first contraction round that answers
from its own records ("prune_one_select").  Each is a choice of schedule or integer selection logic, so every comparison is
bit for bit: records (acq, y, sigma, idx), bounds and arrays with the option on equal those with it off and the full sweep's.

One exception, which is the documented contract of gpry_sweep_topk and not a tolerance: the BOUND of a pruned sweep is >= the
full sweep's (the largest bound of a candidate that was never contracted may stand in for its exact value), so against the
full sweep the bound is checked as >=, and as equal between the two values of an option."""
import numpy as np
import pytest

from gpry_amd import _lib
from oracle import gpry_oracle as orc

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "acq", "y", "sigma")
INFO = ("pruned", "M", "K_prime", "rounds", "contracted", "completed", "K", "survivors", "y_bound", "live_blocks", "blocks")
DEFAULTS = (("sweep_prune", 0), ("topk_host", 16384), ("sweep_small_map", 1), ("select_fused", 1), ("prune_one_select", 1),
            ("timing", 0), ("sweep_chunk", 0))


@pytest.fixture(scope="module")
def dev():
    d = _lib.Device(0)
    yield d
    d.close()


@pytest.fixture(autouse=True)
def _defaults(dev):
    yield
    for k, v in DEFAULTS:
        dev.set_option(k, v)


def _model(N, d, kid, theta, seed=0, noise=1e-2):
    rng = np.random.default_rng(seed)
    bounds = np.array([[-5.0, 5.0]] * d)
    X = rng.uniform(-5, 5, (N, d))
    y = -0.5 * (X ** 2).sum(1)
    m = orc.OracleGPR(bounds, kernel_id=kid, noise_level=noise)
    m.theta = np.asarray(theta, dtype=float)
    m.fitted = True
    m.append_to_data(X, y, fit_gpr=False, fit_preprocessors=True)
    return m


def _load(dev, m):
    dev.set_train(m.X_train_, m.y_train_, m.alpha)
    dev.set_theta(m.kernel_id, m.theta)
    dev.set_affine(m.pre_X.lo, m.pre_X.hi - m.pre_X.lo, m.pre_y.mean_, m.pre_y.std_, m.clip_hi())
    assert dev.factorize() == 0


def _bits(x):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64))).view(np.uint64)


def _same_records(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    np.testing.assert_array_equal(a["idx"], b["idx"], err_msg=f"{what} idx")
    for f in ("acq", "y", "sigma"):
        np.testing.assert_array_equal(_bits(a[f]), _bits(b[f]), err_msg=f"{what} {f}")


def _same_bound(a, b, what=""):
    assert _bits(a)[0] == _bits(b)[0], (what, a, b)


def _stage_a(dev, M, args):
    dev.set_option("sweep_prune", 1)
    try:
        dev.sweep_logexp(None, *args, M=M, want=())
    finally:
        dev.set_option("sweep_prune", 0)


def _info(dev):
    i = dev.sweep_prune_info()
    out = {k: i[k] for k in INFO}
    out["tau"] = _bits(i["tau"])[0]
    return out


# ---- the small-launch tile map ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kid", [orc.MATERN52, orc.RBF])
@pytest.mark.parametrize("N", [2048, 2560, 1100, 700])
def test_small_map_gives_the_full_sweeps_bits(dev, N, kid):
    """N = 2048: two super-rows, both walk directions; 2560: three; 1100: Np = 1152, ragged last super-row; 700: one
    super-row (the map it had already).  K = 64 -> a compact batch of 1024 candidates (8 column tiles), 300 -> 1200 (10, the
    last one ragged), and at N = 2048 K = 1056 -> 4224 (33 x 16 = 528 tiles: the super-tile map)."""
    d, M = 4, 20000
    m = _model(N, d, kid, np.log([1.0, 0.3, 0.3, 0.3, 0.3]), seed=N)
    _load(dev, m)
    dev.set_option("topk_host", 0)
    args = (orc.auto_zeta(d), m.y_max, m.noise_level)
    Xc = np.random.default_rng(N + 1).uniform(-5, 5, (M, d))
    full = dev.sweep_logexp(Xc, *args)
    Ks = [64, 300] + ([1056] if N == 2048 else [])
    ref = {K: dev.sweep_topk(K) for K in Ks}
    for K in Ks:
        got = {}
        for opt in (1, 0):
            dev.set_option("sweep_small_map", opt)
            _stage_a(dev, M, args)
            got[opt] = dev.sweep_topk(K)
            info = _info(dev)
            assert info["K_prime"] >= max(4 * K, 1024) and info["contracted"] >= max(4 * K, 1024), info   # (the compact batch ran)
            _same_records(got[opt][0], ref[K][0], f"N={N} K={K} small_map={opt} against the full sweep")
            assert got[opt][1] >= ref[K][1], (N, K, opt, got[opt][1], ref[K][1])
            arr = dev.sweep_fetch(("y", "sigma", "acq"))        # (the completion)
            for k in ("sigma", "acq", "y"):
                np.testing.assert_array_equal(_bits(arr[k]), _bits(full[k]), err_msg=f"N={N} K={K} small_map={opt} {k}")
        _same_records(got[1][0], got[0][0], f"N={N} K={K} small_map 1 against 0")
        _same_bound(got[1][1], got[0][1], f"N={N} K={K}")


# ---- the select ---------------------------------------------------------------------------------------------------

def _key(acq):
    b = _bits(acq)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def _reference_select(acq, K, exclude):
    """(indices of the shortlist, bits of the bound): the composite order (key desc, idx desc) over the candidates that are
    not excluded; K is capped by M - len(exclude) as given, duplicates and out-of-range entries included."""
    M = len(acq)
    idx = np.arange(M, dtype=np.int64)
    order = np.lexsort((-idx, ~_key(acq)))      # (~key: the descending order of an unsigned key)
    nex = 0 if exclude is None else len(exclude)
    if nex:
        ex = np.asarray(exclude, dtype=np.int64)
        order = order[~np.isin(order, ex[(ex >= 0) & (ex < M)])]
    K = max(0, min(K, M - nex))
    bound = acq[order[K]] if K > 0 and len(order) > K else -np.inf
    return order[:K], _bits(bound)[0]


def _pool(name, M, rng):
    """y of the planted pool; with sigma = 1, noise 0, baseline 0 and zeta = 1/2 the acquisition is y + log(1)."""
    if name == "equal":
        return np.full(M, 0.375)
    if name == "upper40":
        return 1.0 + rng.integers(0, 1 << 24, M) * 2.0 ** -52       # (the upper 40 bits shared)
    y = rng.standard_normal(M)
    if name == "inf":
        y[rng.random(M) < 0.3] = np.inf
        y[rng.random(M) < 0.3] = -np.inf
    elif name == "nan":
        y[rng.random(M) < 0.2] = np.nan
        y[rng.random(M) < 0.1] = np.inf
    elif name == "zeros":       # (whichever zeros the acquisition keeps: the reference orders the device's own array)
        y[:] = 0.0
        y[rng.random(M) < 0.5] = -0.0
        y[rng.random(M) < 0.1] = -1e-300
    return y


@pytest.fixture(scope="module")
def tiny_model(dev):
    return _model(64, 2, orc.MATERN52, np.log([1.0, 0.3, 0.3]), seed=5)


@pytest.mark.parametrize("pool", ["equal", "upper40", "inf", "nan", "zeros", "exclusions"])
def test_fused_select_is_the_scan_select_and_numpy(dev, tiny_model, pool):
    _load(dev, tiny_model)
    dev.set_option("topk_host", 0)
    rng = np.random.default_rng(len(pool))
    for M in (1, 255, 257, 70001):
        y = _pool("upper40" if pool == "exclusions" else pool, M, rng)
        if pool == "exclusions":
            y = np.round(y * 2.0 ** 44) * 2.0 ** -44        # (ties among the best as well)
        Xc = rng.uniform(-5, 5, (M, 2))
        out = dev.sweep_logexp(Xc, 0.5, 0.0, 0.0, y_given=y, sigma_given=np.ones(M))
        acq = out["acq"]
        if pool == "nan":
            assert np.isnan(acq).sum() == np.isnan(y).sum()
        if pool == "zeros":
            assert len(np.unique(_bits(acq))) >= min(M, 2)
        ex = None
        if pool == "exclusions":
            best = np.lexsort((-np.arange(M), ~_key(acq)))[: max(1, M // 3)]
            ex = np.concatenate([best[::2], best[:3], best[:3], [-1, -7, M, M + 5, 2 ** 40]]).astype(np.int64)
        for K in (1, 256, M):
            want_idx, want_bound = _reference_select(acq, K, None if ex is None else np.sort(ex))
            res = {}
            for opt in (1, 0):
                dev.set_option("select_fused", opt)
                top, bound = dev.sweep_topk(K, exclude=ex)
                what = f"pool={pool} M={M} K={K} select_fused={opt}"
                np.testing.assert_array_equal(top["idx"], want_idx, err_msg=what)
                np.testing.assert_array_equal(_bits(top["acq"]), _bits(acq[want_idx]), err_msg=what)
                np.testing.assert_array_equal(_bits(top["y"]), _bits(y[want_idx]), err_msg=what)
                np.testing.assert_array_equal(top["sigma"], np.ones(len(want_idx)), err_msg=what)
                assert _bits(bound)[0] == want_bound, (what, bound)
                res[opt] = (top, bound)
            _same_records(res[1][0], res[0][0], f"pool={pool} M={M} K={K}")
            _same_bound(res[1][1], res[0][1], f"pool={pool} M={M} K={K}")


# ---- one select where the first round answers ---------------------------------------------------------------------

def _one_select_case(dev, Xc, args, calls, expect_shortcut):
    """calls: (K, exclusions), asked in turn of ONE pruned sweep, with the option on and off, and of the full sweep.
    expect_shortcut[i]: True = call i must not run the plain select ("topk" timer), False = it must, None = either."""
    M = len(Xc)
    dev.set_option("topk_host", 0)
    dev.set_option("timing", 1)
    full = dev.sweep_logexp(Xc, *args)
    ref = [dev.sweep_topk(K, exclude=ex) for K, ex in calls]
    res = {}
    for opt in (1, 0):
        dev.set_option("prune_one_select", opt)
        _stage_a(dev, M, args)
        res[opt] = []
        for i, (K, ex) in enumerate(calls):
            n0 = dev.timing("topk")[1]
            top, bound = dev.sweep_topk(K, exclude=ex)
            rose = dev.timing("topk")[1] - n0
            if opt == 1 and expect_shortcut[i] is not None:
                assert (rose == 0) == expect_shortcut[i], (i, K, rose, dev.sweep_prune_info())
            if opt == 0:
                assert rose >= 1 or dev.sweep_prune_info()["completed"] == 1
            res[opt].append((top, bound, _info(dev)))
            _same_records(top, ref[i][0], f"call {i} K={K} prune_one_select={opt} against the full sweep")
            assert bound >= ref[i][1], (i, K, opt, bound, ref[i][1])
        arr = dev.sweep_fetch(("y", "sigma", "acq"))
        for k in ("y", "sigma", "acq"):
            np.testing.assert_array_equal(_bits(arr[k]), _bits(full[k]), err_msg=f"prune_one_select={opt} {k}")
    for i, (a, b) in enumerate(zip(res[1], res[0])):
        _same_records(a[0], b[0], f"call {i}: option on against off")
        _same_bound(a[1], b[1], f"call {i}")
        assert a[2] == b[2], (i, a[2], b[2])
    return res


@pytest.fixture(scope="module")
def near_pool():
    d, M = 4, 20000
    m = _model(700, d, orc.MATERN52, np.log([1.0, 0.3, 0.3, 0.3, 0.3]), seed=9)
    Xc = np.random.default_rng(10).uniform(-5, 5, (M, d))
    # (zeta = 20: the mean decides the ranking by far more than the bound of sigma can move it, so round 1 answers)
    return m, Xc, (20.0, m.y_max, m.noise_level)


def test_first_round_answers_without_a_second_select(dev, near_pool):
    m, Xc, args = near_pool
    _load(dev, m)
    res = _one_select_case(dev, Xc, args, [(64, None)], [True])
    assert res[1][0][2]["rounds"] == 1 and res[1][0][2]["contracted"] == 1024, res[1][0][2]


def test_second_call_on_the_same_sweep_takes_the_plain_select(dev, near_pool):
    m, Xc, args = near_pool
    _load(dev, m)
    _one_select_case(dev, Xc, args, [(64, None), (256, None)], [True, False])


def test_exclusions_that_remove_some_of_the_best(dev, near_pool):
    m, Xc, args = near_pool
    _load(dev, m)
    dev.set_option("topk_host", 0)
    a = dev.sweep_logexp(Xc, *args)["acq"]
    best = np.lexsort((-np.arange(len(a)), ~_key(a)))[:40]
    _one_select_case(dev, Xc, args, [(64, best[::3])], [None])


def test_fewer_valid_candidates_than_k(dev, near_pool):
    m, Xc, args = near_pool
    _load(dev, m)
    M = len(Xc)
    ex = np.arange(30, M)                      # 30 candidates count, 64 asked for
    res = _one_select_case(dev, Xc, args, [(64, ex)], [None])
    assert len(res[1][0][0]) == 30


def test_tie_with_the_outside_bound_falls_back(dev):
    """The pool of tests/test_sweep_exactness_gpu.py::test_tie_pool_of_far_candidates_at_the_kth_place: 3000 far candidates
    whose acquisition equals its bound bit for bit, above near ones whose bounds are lower.  A shortlist of 256 (or of 1)
    contracts the 1024 far rows of highest index in round 1; its 256th (1st) exact value then EQUALS the best bound outside
    (the next far row's), so the strict comparison fails and the plain select must run."""
    d = 3
    m = _model(300, d, orc.MATERN52, np.log([1.0, 0.3, 0.3, 0.3]))
    _load(dev, m)
    y_mean, y_std = m.pre_y.mean_, m.pre_y.std_
    sn = np.sqrt(0.9) * y_std
    args = (orc.auto_zeta(d), y_mean, sn)
    rng = np.random.default_rng(3)
    n_near = 36000
    cand = rng.uniform(-5, 5, (100000, d))
    yc = dev.sweep_logexp(cand, *args, want=("y",))["y"]
    near = cand[yc < y_mean - 1e-3 * y_std][:n_near]
    assert len(near) == n_near
    far = 5.0 + 1e4 + rng.uniform(0, 10, (3000, d))
    Xc = np.concatenate([near, far])
    a = dev.sweep_logexp(Xc, *args)["acq"]
    assert np.all(a[n_near:] == a[n_near]) and not (a[:n_near] >= a[n_near]).any()
    res = _one_select_case(dev, Xc, args, [(256, None)], [False])
    assert res[1][0][2]["rounds"] == 1 and res[1][0][2]["contracted"] == 1024, res[1][0][2]
    _one_select_case(dev, Xc, args, [(1, None)], [False])
