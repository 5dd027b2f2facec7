"""The pruned sweep (option "sweep_prune", sweep_topk.hip: prune_topk) against the full sweep on the same model and pool: the
shortlist records (idx, acq, y, sigma) are equal bit for bit, the pruned bound is >= the full one, and every array fetched
after a pruned shortlist is the full sweep's.  NORA.multi_add gives the same proposals with exact_prune on and off."""
import numpy as np
import pytest

from oracle import gpry_oracle as orc
from test_host_mirror_gpu import make_gpr

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "acq", "y", "sigma")


def _model(N, d, M, kid, theta, seed=0):
    bounds, X, y, Xc = orc.synthetic_problem(N, d, M, seed_train=seed)
    gpr = make_gpr(bounds, kid, theta=np.asarray(theta, dtype=float))
    gpr.append_to_data(X, y, fit_gpr=False)
    gpr._ensure_factor()
    gpr._push_affine()
    return bounds, Xc, gpr


def _sweep(dev, X, gpr, prune, mask=None, M=None):
    zeta = orc.auto_zeta(gpr.d)
    dev.set_option("sweep_prune", int(prune))
    try:
        out = dev.sweep_logexp(X, zeta, gpr.y_max, gpr.noise_level, mask=mask, M=M, want=())
    finally:
        dev.set_option("sweep_prune", 0)
    assert out["n_nan"] == 0
    return out


def _compare(dev, Xc, gpr, K, exclude=None, mask=None, check_fetch=True):
    """Full sweep, then the pruned one of the same (resident) pool: shortlists and the arrays fetched afterwards."""
    _sweep(dev, Xc, gpr, False, mask=mask)
    full = dev.sweep_fetch(("y", "sigma", "acq"))
    ft, fb = dev.sweep_topk(K, exclude=exclude)
    _sweep(dev, None, gpr, True, mask=mask, M=len(Xc))
    pt, pb = dev.sweep_topk(K, exclude=exclude)
    info = dev.sweep_prune_info()
    for f in FIELDS:
        np.testing.assert_array_equal(pt[f], ft[f], err_msg=f)
    assert pb >= fb, (pb, fb)
    if check_fetch:
        got = dev.sweep_fetch(("y", "sigma", "acq"))
        for k in ("y", "sigma", "acq"):
            np.testing.assert_array_equal(got[k], full[k], err_msg=k)
        assert dev.sweep_prune_info()["pruned"] == 0
    return full, info


def _theta_bench_like(d):
    return np.log(np.array([4.0] + [0.3] * d))


@pytest.mark.timeout(900)
def test_config2_size_theta_03_prunes_and_matches_the_full_sweep():
    N, d, M = 4096, 16, 1_000_000
    bounds, Xc, gpr = _model(N, d, M, orc.MATERN52, _theta_bench_like(d))
    dev = gpr.device
    full, info = _compare(dev, Xc, gpr, 256, check_fetch=False)
    surv = info["survivors"] if info["survivors"] >= 0 else info["K_prime"]
    print(f"theta = log[4, 0.3...], N = {N}, M = {M}: survivors of the threshold {surv} ({surv / M:.3%}), "
          f"contracted {info['contracted']}, K' = {info['K_prime']}, rounds {info['rounds']}, completed {info['completed']}")
    assert info["completed"] == 0 and 0 < surv < 0.25 * M       # (11 % when measured)
    # a later shortlist 4x as long: answered from the contracted set or by completing; same records either way
    a = full["acq"]
    order = np.lexsort((-np.arange(M), -a))
    top, bound = dev.sweep_topk(1024)
    np.testing.assert_array_equal(top["idx"], order[:1024])
    np.testing.assert_array_equal(top["acq"], a[order[:1024]])
    assert bound >= a[order[1024]]
    # the fetch completes: the full sweep's arrays, and after it the full sweep's bound
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(got[k], full[k], err_msg=k)
    top, bound = dev.sweep_topk(256)
    assert bound == a[order[256]]


@pytest.mark.timeout(900)
def test_bench_fitted_model_prunes_and_matches_the_full_sweep():
    import bench
    N, d, M = 4096, 16, 1_000_000
    bounds, X, y, Xc, truth = bench.synthetic(N - d, d, M)
    gpr = bench.make_gpr(bounds)
    gpr.append_to_data(X, y, fit_gpr="simple")
    gpr._ensure_factor()
    gpr._push_affine()
    dev = gpr.device
    _, info = _compare(dev, Xc, gpr, 256)
    frac = info["contracted"] / M
    print(f"bench model, N = {gpr.n}, M = {M}: contracted {info['contracted']} ({frac:.3%}), K' = {info['K_prime']}, "
          f"rounds {info['rounds']}, survivors {info['survivors']}, completed {info['completed']}")
    assert info["pruned"] == 1 and info["completed"] == 0 and frac < 1.0


def test_config1_rbf_d8_matches_the_full_sweep():
    N, d, M = 1024, 8, 100_000
    bounds, Xc, gpr = _model(N, d, M, orc.RBF, np.log(np.array([1.0] + [0.6] * d)))
    _compare(gpr.device, Xc, gpr, 256)


def test_ties_across_the_kth_place():
    N, d = 512, 4
    bounds, Xc, gpr = _model(N, d, 60_000, orc.MATERN52, np.log(np.array([2.0] + [0.3] * d)))
    dev = gpr.device
    _sweep(dev, Xc, gpr, False)
    a = dev.sweep_fetch(("acq",))["acq"]
    best = np.argsort(a)[::-1][:300]
    Xd = np.concatenate([Xc, Xc[best], Xc[best[::-1]]])          # every one of the 300 best three times
    _compare(dev, Xd, gpr, 256)
    _compare(dev, Xd, gpr, 257)


def test_masked_rows():
    N, d, M = 512, 4, 60_000
    bounds, Xc, gpr = _model(N, d, M, orc.MATERN32, np.log(np.array([2.0] + [0.3] * d)))
    dev = gpr.device
    _sweep(dev, Xc, gpr, False)
    a = dev.sweep_fetch(("acq",))["acq"]
    best = np.argsort(a)[::-1][:400]
    mask = np.zeros(M, np.uint8)
    mask[best[::3]] = 2                     # outside the trust region: y = -inf
    mask[best[1::3]] = 1                    # classified infinite: y = -inf, sigma = 0
    mask[np.random.default_rng(1).choice(M, 5000, replace=False)] = 1
    full, _ = _compare(dev, Xc, gpr, 256, mask=mask)
    assert np.isneginf(full["acq"][mask != 0]).all()


def test_pool_smaller_than_the_shortlist_and_exclusions():
    N, d = 512, 4
    bounds, Xc, gpr = _model(N, d, 60_000, orc.MATERN52, np.log(np.array([2.0] + [0.3] * d)))
    dev = gpr.device
    _compare(dev, Xc[:200], gpr, 256)
    _sweep(dev, Xc, gpr, False)
    a = dev.sweep_fetch(("acq",))["acq"]
    ex = np.sort(np.argsort(a)[::-1][:40:3])
    _compare(dev, Xc, gpr, 256, exclude=ex)


def _nora_runs(bounds, Xc, make, devices, prune, calls=3):
    from gpry_amd.gp_acquisition import NORA
    gpr = make()
    acq = NORA(bounds, sampler="uniform", mc_every=2, verbose=0, devices=devices, exact_prune=prune)
    acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
    rng = np.random.default_rng(2)
    res = []
    for _ in range(calls):
        Xp, yp, ap = acq.multi_add(gpr, n_points=4, rng=rng)
        res.append((Xp, yp, ap, acq.stats.get("prune")))
        gpr.append_to_data(Xp, np.sum(Xp, axis=1), fit_gpr=False)
    s = acq.last_MC_sample(warn_reweight=False)
    return res, s


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
def test_multi_add_with_and_without_pruning(devices):
    N, d, M = 1024, 6, 200_000
    bounds, X, y, Xc = orc.synthetic_problem(N, d, M)
    theta = np.log(np.array([2.0] + [0.25] * d))

    def make():
        gpr = make_gpr(bounds, orc.MATERN52, theta=theta)
        gpr.append_to_data(X, y, fit_gpr=False)
        return gpr

    on, s_on = _nora_runs(bounds, Xc, make, devices, True)
    off, s_off = _nora_runs(bounds, Xc, make, devices, False)
    for (a, b) in zip(on, off):
        for u, v in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(u, v)
        assert b[3] is None
    assert on[0][3] is not None and len(on[0][3]) == len(devices)
    assert all(p["M"] > 0 and p["K_prime"] > 0 and p["rounds"] >= 1 for p in on[0][3]), on[0][3]   # every member pruned
    assert on[1][3] is None                 # the second call of mc_every = 2 re-weights: a full sweep
    for u, v in zip(s_on, s_off):
        if u is not None:
            np.testing.assert_array_equal(u, v)


def test_model_change_after_a_pruned_sweep_keeps_the_sweeps_model():
    """A refactorisation with another theta between the pruned sweep and its shortlist / fetch: both still answer for the
    model the sweep was made with (the context keeps a copy of it), as the stored arrays of a full sweep would."""
    N, d, M = 512, 4, 60_000
    theta1 = np.log(np.array([2.0] + [0.3] * d))
    bounds, Xc, gpr = _model(N, d, M, orc.MATERN52, theta1)
    dev = gpr.device
    _sweep(dev, Xc, gpr, False)
    full = dev.sweep_fetch(("y", "sigma", "acq"))
    ft, fb = dev.sweep_topk(256)
    f4, fb4 = dev.sweep_topk(2048)
    _sweep(dev, None, gpr, True, M=M)
    kid, _ = gpr._device_theta()
    dev.set_theta(kid, np.log(np.array([3.0] + [0.7] * d)))
    assert dev.factorize() == 0
    pt, pb = dev.sweep_topk(256)
    p4, pb4 = dev.sweep_topk(2048)
    for f in FIELDS:
        np.testing.assert_array_equal(pt[f], ft[f], err_msg=f)
        np.testing.assert_array_equal(p4[f], f4[f], err_msg=f)
    assert pb >= fb and pb4 >= fb4
    got = dev.sweep_fetch(("y", "sigma", "acq"))
    for k in ("y", "sigma", "acq"):
        np.testing.assert_array_equal(got[k], full[k], err_msg=k)


@pytest.mark.timeout(900)
def test_refit_then_reweight_and_last_sample_on_the_bench_model():
    """The ordinary cycle with re-weighting (mc_every = 2) on the bench's model, where the first contraction round answers
    alone: multi_add -> append_to_data (refit, refactorisation) -> last_MC_sample -> re-weighted multi_add.  Everything
    equals the run without pruning."""
    import bench
    from gpry_amd.gp_acquisition import NORA
    N, d, M = 4096, 16, 1_000_000
    bounds, X, y, Xc, truth = bench.synthetic(N - d, d, M)
    res = {}
    for prune in (True, False):
        gpr = bench.make_gpr(bounds)
        gpr.append_to_data(X, y, fit_gpr="simple")
        acq = NORA(bounds, sampler="uniform", mc_every=2, verbose=0, devices=[0], exact_prune=prune)
        acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc, None, None, None)
        rng = np.random.default_rng(2)
        first = acq.multi_add(gpr, n_points=d, rng=rng)
        st = acq.stats.get("prune")
        if prune:
            assert st[0]["pruned"] == 1 and st[0]["completed"] == 0 and st[0]["K_prime"] < M // 100, st
        else:
            assert st is None
        gpr.append_to_data(first[0], truth(first[0]), fit_gpr="simple")
        sample = [np.copy(v) for v in acq.last_MC_sample(warn_reweight=False)[:3]]
        second = acq.multi_add(gpr, n_points=d, rng=rng)
        rw = [np.copy(v) for v in acq.last_MC_sample(warn_reweight=False)]
        res[prune] = (first, sample, second, rw)
    for a, b in zip(res[True], res[False]):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
