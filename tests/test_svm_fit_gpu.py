"""gpry_svm_fit on the GPU (``Device.svm_fit``, ``SVM(trainer="device")``) against scikit-learn's SVC computed here, with
the tolerances derived in tests/tools/svm_smo_numpy.py (``bounds``): feasibility, the stop test and the objective recomputed
on the host, decision values and verdicts, training labels; the bits (two contexts, the launch length, a context that
holds a model, a sweep and a Kriging-believer session); the iteration budget and the classifier's fallback; the refusals;
and a regressor whose classifier trains on the device, through ``append_to_data``, ``predict`` (the device's gates) and
``NORA.multi_add``, against a twin with the default trainer.

Shapes: the wave edge (63, 64, 65), the workgroup stride (1023, 1024, 1025), every points-per-thread instantiation
(<= 1024, 2049, 4097 -> 1, 2, 4 x 1024 threads and 16 x 512 threads), N = 2 and 3; d = 1, 2, 16, 17, 32 (the padding of the
coordinate-major copy to a multiple of four).  d = 2 goes with N = 3 and N = 65 and not with the large separable sets: at
(1024, 2), C = 1e7 the alphas reach 1e3 and libsvm's own solution, asked for tol = 1e-10, misses the stop test by 1.2e-4
when its gradient is recomputed (and lies 9.5e-6 above this solver's objective, where eps S is 1.9e-6) -- it cannot be the
reference for bounds that presuppose a reference converged to eps.  On the sets used here its recomputed violation is
5e-7 to 2e-5, and the gaps stay two orders of magnitude inside eps S."""
import os
import sys

import numpy as np
import pytest
from sklearn.svm import SVC

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import svm_smo_numpy as sn  # noqa: E402
import sampler_walk as sw  # noqa: E402
from gpry_amd.svm import SVM  # noqa: E402

pytestmark = pytest.mark.gpu

M_TEST = 4000
# (N, d, separable, eps): C = 1e7 on the separable sets, 10 on the overlapping ones
CASES = [(2, 1, True, 1e-10), (3, 2, True, 1e-10), (63, 16, True, 1e-10), (64, 17, False, 1e-10), (65, 32, True, 1e-10),
         (1023, 1, False, 1e-10), (1024, 32, True, 1e-10), (1025, 16, True, 1e-10), (2049, 17, False, 1e-10),
         (4097, 32, True, 1e-10), (65, 2, True, 1e-3), (1025, 17, True, 1e-3), (2049, 16, True, 1e-3), (4097, 16, True, 1e-3)]
_cache = {}
_devices = {}


def _device(name="main"):
    from gpry_amd import _lib
    if name not in _devices:
        _devices[name] = _lib.Device(0)
    return _devices[name]


def _data(N, d, separable):
    X, finite = sn.labelled_set(N, d, seed=N + d, separable=separable)
    return X, finite, (1e7 if separable else 10.0), 1.0 / (d * X.var())


def _case(N, d, separable, eps):
    key = (N, d, separable, eps)
    if key not in _cache:
        X, finite, C, gamma = _data(N, d, separable)
        res = _device().svm_fit(X, finite, C, gamma, eps=eps)
        svc = SVC(C=C, kernel="rbf", gamma=gamma, tol=eps).fit(X, finite)
        a_sk = np.zeros(N)
        a_sk[svc.support_] = np.abs(svc.dual_coef_[0])
        _cache[key] = dict(X=X, finite=finite, y=np.where(finite, 1.0, -1.0), C=C, gamma=gamma, res=res, svc=svc, a_sk=a_sk,
                           mine=sn.host_checks(X, finite, res["alpha"], gamma, C), theirs=sn.host_checks(X, finite, a_sk, gamma, C),
                           b=sn.bounds(res["alpha"], a_sk, eps, d, res["n_iter"]))
    return _cache[key]


@pytest.mark.parametrize("N,d,separable,eps", CASES)
def test_solution_against_libsvm(N, d, separable, eps):
    c = _case(N, d, separable, eps)
    res, b, mine = c["res"], c["b"], c["mine"]
    alpha = res["alpha"]
    gap = abs(mine["objective"] - c["theirs"]["objective"])
    print(f"iterations {res['n_iter']} (libsvm {int(np.max(c['svc'].n_iter_))}), {mine['n_sv']} support vectors, device {res['device_ms']:.3f} ms; "
          f"violation {res['violation']:.3e} host {mine['violation']:.3e} (rounding {b['grad_round']:.3e}); "
          f"|sum y alpha| {abs(mine['sum_y_alpha']):.3e} <= {b['equality']:.3e}; objective gap {gap:.3e} <= {b['objective']:.3e}")
    assert res["status"] == 0 and res["n_iter"] >= 1
    assert np.all(alpha >= 0.0) and np.all(alpha <= c["C"])                     # exactly
    assert abs(mine["sum_y_alpha"]) <= b["equality"]
    assert res["violation"] < eps                                               # the device's test, on its recomputed gradient
    assert mine["violation"] <= eps + 2.0 * b["grad_round"]                     # the same from scratch on the host
    assert gap <= b["objective"]
    # the device's own objective 1/2 sum alpha (G - 1): both gradients carry grad_round per entry, the sums their rounding
    assert abs(res["objective"] - mine["objective"]) <= (2.0 * b["grad_round"] * np.sum(alpha)
                                                           + N * 2.0 ** -53 * np.sum(alpha * np.abs(mine["G"] - 1.0)))
    if not separable:
        assert np.count_nonzero(alpha >= c["C"]) > 0
    dec_train = sn.decision(c["X"], c["X"], c["y"], alpha, res["rho"], c["gamma"])
    if separable:
        assert np.array_equal(dec_train > 0.0, c["finite"])
    if eps == 1e-10:
        Xt = sn.probe_points(c["X"], M_TEST, seed=5)
        dec, dec_sk = sn.decision(Xt, c["X"], c["y"], alpha, res["rho"], c["gamma"]), c["svc"].decision_function(Xt)
        outside = np.abs(dec_sk) > b["decision"]
        print(f"decision diff {np.max(np.abs(dec - dec_sk)):.3e} <= B = {b['decision']:.3e}; {np.count_nonzero(~outside)} of {M_TEST} inside B")
        assert np.max(np.abs(dec - dec_sk)) <= b["decision"]
        assert np.count_nonzero(~outside) <= 0.01 * M_TEST
        assert np.array_equal((dec > 0.0)[outside], (dec_sk > 0.0)[outside])


def _same_bits(a, b):
    assert np.array_equal(a["alpha"], b["alpha"]) and a["rho"] == b["rho"] and a["n_iter"] == b["n_iter"]
    assert a["objective"] == b["objective"] and a["violation"] == b["violation"] and a["status"] == b["status"]


@pytest.mark.parametrize("N,d,separable,eps", [(1025, 16, True, 1e-10), (2049, 17, False, 1e-10)])
def test_bits_do_not_depend_on_context_or_launch_length(N, d, separable, eps):
    c = _case(N, d, separable, eps)
    other = _device("second")
    _same_bits(other.svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=eps), c["res"])
    assert c["res"]["n_iter"] > 64
    try:
        other.set_option("svm_iters_per_launch", 64)
        _same_bits(other.svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=eps), c["res"])
        cut = other.svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=eps, max_iter=100)     # the budget ends inside a launch
    finally:
        other.set_option("svm_iters_per_launch", 4096)
    assert other.get_option("svm_iters_per_launch") == 4096
    _same_bits(cut, _device().svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=eps, max_iter=100))
    assert cut["status"] == 1 and cut["n_iter"] == 100


def test_context_with_model_sweep_and_session_gives_the_same_bits_and_keeps_them():
    model = sw.Model(4, sw.M52, 200, seed=3)
    gpr = model.gpr()
    gpr._ensure_factor()
    gpr._push_affine()
    dev = gpr.device
    Xc = np.random.default_rng(1).uniform(model.bounds[:, 0], model.bounds[:, 1], (3000, 4))

    def state():
        mean, std = dev.predict(Xc[:300], return_std=True)
        fetched = dev.sweep_fetch(want=("y", "sigma"))
        G, kvec = dev.kb_gram(2, 8)
        top, bound = dev.sweep_topk(5)
        return [mean, std, fetched["y"], fetched["sigma"], G, kvec, np.frombuffer(top.tobytes(), dtype=np.uint8), bound]

    dev.sweep_logexp(Xc, 0.3, gpr.y_max, gpr.noise_level)
    dev.kb_reset()
    dev.kb_register(Xc[:8])
    before = state()
    c = _case(1025, 16, True, 1e-10)
    _same_bits(dev.svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=1e-10), c["res"])
    for a, b in zip(before, state()):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_budget_is_a_status_and_the_classifier_falls_back():
    c = _case(1025, 16, True, 1e-10)
    res = _device().svm_fit(c["X"], c["finite"], c["C"], c["gamma"], eps=1e-10, max_iter=10)
    assert res["status"] == 1 and res["n_iter"] == 10
    alpha = res["alpha"]
    assert np.all(alpha >= 0.0) and np.all(alpha <= c["C"]) and np.count_nonzero(alpha) >= 2
    assert abs(np.sum(c["y"] * alpha)) <= 2.0 * 10 * 2.0 ** -53 * np.max(alpha)
    y = np.where(c["finite"], -np.linspace(0.0, 5.0, 1025), -np.inf)
    svm = SVM(trainer="device", tol=1e-10, max_iter=10).bind(_device())
    ref = SVM(tol=1e-10, max_iter=10)
    for s in (svm, ref):
        assert np.array_equal(s.fit(c["X"], y, 10.0), c["finite"])
    assert svm.fit_info["trainer_used"] == "libsvm" and svm.fit_info["status"] == 1 and svm.fit_info["n_iter"] == 10
    for a, b in zip(svm.device_params(), ref.device_params()):
        assert np.array_equal(a, b)


def test_refusals():
    dev = _device()
    X, finite, C, gamma = _data(64, 2, True)
    for Xb, fb in ((X, np.ones(64, bool)), (X, np.zeros(64, bool)), (X[:1], finite[:1]),
                   (np.zeros((8193, 2)), np.arange(8193) % 2 == 0), (np.where(np.arange(128).reshape(64, 2) == 5, np.nan, X), finite),
                   (np.where(np.arange(128).reshape(64, 2) == 7, np.inf, X), finite), (np.zeros((64, 33)), finite)):
        with pytest.raises(RuntimeError, match="gpry_svm_fit"):
            dev.svm_fit(Xb, fb, C, gamma)
    for kw in (dict(C=np.inf), dict(C=0.0), dict(gamma=np.nan), dict(gamma=-1.0), dict(eps=0.0)):
        args = dict(C=C, gamma=gamma, eps=1e-3)
        args.update(kw)
        with pytest.raises(RuntimeError, match="gpry_svm_fit"):
            dev.svm_fit(X, finite, **args)
    assert dev.svm_fit(X, finite, C, gamma)["status"] == 0          # the context is fine afterwards


def test_gpr_with_a_device_trained_classifier_end_to_end():
    """append_to_data (which holds the reference's assertion on the labels), predict -- its -inf are the verdicts of the
    device's gates, fed from device_params() of the device-trained classifier -- and a small NORA.multi_add, against a twin
    with the default trainer, at every candidate whose libsvm decision value lies outside B."""
    from gpry_amd.gp_acquisition import NORA
    d, N, eps = 3, 300, 1e-10
    model = sw.Model(d, sw.M52, N, seed=9)
    y = model.y.copy()
    y[model.X[:, 0] > 1.5] = -np.inf
    kw = dict(inf_threshold="20s", random_state=1)
    gpr = sw.mirror(model.bounds, model.kid, model.theta, account_for_inf=SVM(trainer="device", tol=eps), **kw)
    twin = sw.mirror(model.bounds, model.kid, model.theta, account_for_inf=SVM(tol=eps), **kw)
    for g in (gpr, twin):
        g.append_to_data(model.X, y, fit_gpr=False)
    clf, ref = gpr.infinities_classifier, twin.infinities_classifier
    assert clf.fit_info["trainer_used"] == "device" and clf.fit_info["status"] == 0 and clf._svc is None
    assert ref.fit_info["trainer_used"] == "libsvm" and clf._dev is gpr.device
    assert np.array_equal(clf.y_finite, ref.y_finite)
    Xc = np.random.default_rng(4).uniform(model.bounds[:, 0], model.bounds[:, 1], (M_TEST, d))
    X_ = gpr.preprocessing_X.transform(Xc)
    b = sn.bounds(np.abs(clf.device_params()[1]), np.abs(ref.device_params()[1]), eps, d, clf.fit_info["n_iter"])
    rdec, dec = ref.decision_function(X_), clf.decision_function(X_)
    outside = np.abs(rdec) > b["decision"]
    print(f"B = {b['decision']:.3e}; {np.count_nonzero(~outside)} of {M_TEST} inside; decision diff {np.max(np.abs(dec - rdec)):.3e}")
    assert np.count_nonzero(~outside) <= 0.01 * M_TEST and np.max(np.abs(dec - rdec)) <= b["decision"]
    m, mt = gpr.predict(Xc), twin.predict(Xc)
    assert gpr._dev_gates is not None and gpr._dev_gates[1], "predict did not leave the classifier to the device's gates"
    assert np.array_equal(np.isneginf(m)[outside], (dec <= 0.0)[outside])       # the gates against decision_function > 0
    assert np.array_equal(np.isneginf(m)[outside], np.isneginf(mt)[outside])
    assert 100 < np.isneginf(m).sum() < M_TEST - 100
    keep = outside & ~np.isneginf(m)
    np.testing.assert_allclose(m[keep], mt[keep], rtol=1e-9, atol=1e-9)
    res = []
    for g in (gpr, twin):
        acq = NORA(model.bounds, sampler="uniform", verbose=0)
        acq.do_MC_sample = lambda gpr, bounds=None, rng=None, sampler=None: (Xc[outside], None, None, None)
        res.append(acq.multi_add(g, n_points=3, rng=np.random.default_rng(0)))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-6, atol=1e-9)
