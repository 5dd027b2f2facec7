"""The device trainer of the infinities classifier without a GPU: tests/tools/svm_smo_numpy.py -- the order of operations
of gpry_svm_fit in numpy -- against scikit-learn's SVC (libsvm) on separable sets (C = 1e7) and on overlapping ones
(C = 10, which reaches the clipping branches), with the tolerances derived in that file's ``bounds``; and the ``SVM`` class
with ``trainer="device"`` on a numpy device built from the restatement: ``device_params``, ``decision_function``,
``predict``, pickling, ``fit_info``, the three fallbacks to libsvm, and a regressor whose classifier trains that way
through ``append_to_data``."""
import os
import pickle
import sys

import numpy as np
import pytest
from sklearn.svm import SVC

from conftest import ROOT
from oracle_device import OracleDevice

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import svm_smo_numpy as sn  # noqa: E402
import sampler_walk as sw  # noqa: E402
from gpry_amd.svm import SVM  # noqa: E402

EPS = 1e-10
M_TEST = 4000


class NumpyDevice(sn.NumpySvmFit, OracleDevice):
    """The oracle-backed device with the trainer's call; counts its fits."""
    n_svm_fit = 0

    def svm_fit(self, *a, **kw):
        self.n_svm_fit += 1
        return super().svm_fit(*a, **kw)


# every N and every d of the issue once or more; (N, d, separable)
CASES = [(2, 1, True), (3, 2, True), (64, 2, True), (64, 17, False), (257, 8, True), (257, 1, False), (1024, 8, True),
         (1024, 17, False)]
_cache = {}


def _case(N, d, separable):
    """The restatement's fit, scikit-learn's and everything derived from the two (computed once per case)."""
    key = (N, d, separable)
    if key not in _cache:
        X, finite = sn.labelled_set(N, d, seed=N + d, separable=separable)
        C = 1e7 if separable else 10.0
        gamma = 1.0 / (d * X.var())
        res = sn.svm_fit(X, finite, C, gamma, eps=EPS)
        svc = SVC(C=C, kernel="rbf", gamma=gamma, tol=EPS).fit(X, finite)
        a_sk = np.zeros(N)
        a_sk[svc.support_] = np.abs(svc.dual_coef_[0])
        Xt = sn.probe_points(X, M_TEST, seed=5)
        y = np.where(finite, 1.0, -1.0)
        _cache[key] = dict(X=X, finite=finite, y=y, C=C, gamma=gamma, res=res, svc=svc, a_sk=a_sk, Xt=Xt,
                           mine=sn.host_checks(X, finite, res["alpha"], gamma, C), theirs=sn.host_checks(X, finite, a_sk, gamma, C),
                           b=sn.bounds(res["alpha"], a_sk, EPS, d, res["n_iter"]),
                           dec=sn.decision(Xt, X, y, res["alpha"], res["rho"], gamma), dec_sk=svc.decision_function(Xt))
    return _cache[key]


@pytest.mark.parametrize("N,d,separable", CASES)
def test_feasible_and_stopped_on_a_recomputed_gradient(N, d, separable):
    c = _case(N, d, separable)
    res, b = c["res"], c["b"]
    alpha = res["alpha"]
    assert res["status"] == 0 and res["n_iter"] >= 1
    assert np.all(alpha >= 0.0) and np.all(alpha <= c["C"])
    assert abs(c["mine"]["sum_y_alpha"]) <= b["equality"]
    assert res["violation"] < EPS                                   # the solver's own test, on its recomputed gradient
    print(f"violation {res['violation']:.3e} host {c['mine']['violation']:.3e} rounding {b['grad_round']:.3e}")
    assert c["mine"]["violation"] <= EPS + 2.0 * b["grad_round"]    # the same from scratch on the host
    if not separable:
        assert np.count_nonzero(alpha >= c["C"]) > 0, "the overlapping set reaches no bound: the clipping branches are not covered"


@pytest.mark.parametrize("N,d,separable", CASES)
def test_objective_and_decision_values_against_libsvm(N, d, separable):
    c = _case(N, d, separable)
    b = c["b"]
    gap = abs(c["mine"]["objective"] - c["theirs"]["objective"])
    diff = np.max(np.abs(c["dec"] - c["dec_sk"]))
    outside = np.abs(c["dec_sk"]) > b["decision"]
    print(f"objective gap {gap:.3e} <= {b['objective']:.3e}; decision diff {diff:.3e} <= B = {b['decision']:.3e}; "
          f"{np.count_nonzero(~outside)} of {M_TEST} inside B; iterations {c['res']['n_iter']} (libsvm {int(np.max(c['svc'].n_iter_))})")
    assert gap <= b["objective"]
    assert diff <= b["decision"]
    assert np.count_nonzero(~outside) <= 0.01 * M_TEST
    assert np.array_equal((c["dec"] > 0.0)[outside], (c["dec_sk"] > 0.0)[outside])


@pytest.mark.parametrize("N,d,separable", [k for k in CASES if k[2]])
def test_training_labels_reproduced_on_separable_sets(N, d, separable):
    c = _case(N, d, separable)
    dec = sn.decision(c["X"], c["X"], c["y"], c["res"]["alpha"], c["res"]["rho"], c["gamma"])
    assert np.array_equal(dec > 0.0, c["finite"])


def test_budget_is_a_status_and_alpha_stays_feasible():
    X, finite = sn.labelled_set(257, 8, seed=265)
    res = sn.svm_fit(X, finite, 1e7, 1.0 / (8 * X.var()), eps=EPS, max_iter=10)
    assert res["status"] == 1 and res["n_iter"] == 10
    assert np.all(res["alpha"] >= 0.0) and abs(np.sum(np.where(finite, 1.0, -1.0) * res["alpha"])) <= 1e-12 * np.max(res["alpha"])


def test_refusals():
    X, finite = sn.labelled_set(64, 2, seed=66)
    g = 1.0
    for bad in ((X[:1], finite[:1]), (X, np.ones(64, bool)), (np.zeros((8193, 2)), np.arange(8193) % 2 == 0),
                (np.where(np.arange(128).reshape(64, 2) == 5, np.nan, X), finite), (np.zeros((64, 33)), finite)):
        with pytest.raises(RuntimeError):
            sn.svm_fit(bad[0], bad[1], 1e7, g)
    with pytest.raises(RuntimeError):
        sn.svm_fit(X, finite, np.inf, g)


# ---- the SVM class on a numpy device ----------------------------------------------------------------------------------
def _targets(X, finite):
    """Targets whose threshold labels are ``finite`` (diff_threshold 10 below the maximum 0)."""
    return np.where(finite, -np.linspace(0.0, 5.0, len(X)), -np.inf)


def _trained(trainer, N=257, d=8, tol=EPS, device=None, **kw):
    X, finite = sn.labelled_set(N, d, seed=N + d)
    svm = SVM(trainer=trainer, tol=tol, **kw)
    if device is not None:
        svm.bind(device)
    labels = svm.fit(X, _targets(X, finite), 10.0)
    assert np.array_equal(labels, finite)
    return svm, X, finite


def test_svm_class_device_trainer_matches_the_default_one():
    dev = NumpyDevice()
    svm, X, finite = _trained("device", device=dev)
    ref, _, _ = _trained("libsvm")
    assert dev.n_svm_fit == 1 and svm._svc is None
    info = svm.fit_info
    assert info["trainer_used"] == "device" and info["status"] == 0 and info["n_iter"] > 0 and info["fallback"] is None
    assert info["violation"] < EPS and info["objective"] < 0.0 and info["device_ms"] == 0.0
    assert ref.fit_info["trainer_used"] == "libsvm"
    sv, coef, gamma, intercept, pos = svm.device_params()
    rsv, rcoef, rgamma, rintercept, rpos = ref.device_params()
    assert pos is True and rpos is True and gamma == pytest.approx(rgamma, rel=1e-14) == pytest.approx(1.0 / (8 * X.var()), rel=1e-14)
    assert sv.shape == rsv.shape and np.array_equal(sv, X[svm._fit["support"]])
    assert np.all(coef[finite[svm._fit["support"]]] > 0.0) and np.all(coef[~finite[svm._fit["support"]]] < 0.0)
    b = sn.bounds(np.abs(coef), np.abs(rcoef), EPS, 8, info["n_iter"])
    Xt = sn.probe_points(X, M_TEST, seed=7)
    dec, rdec = svm.decision_function(Xt), ref.decision_function(Xt)
    assert np.array_equal(rdec, ref._svc.decision_function(Xt))
    np.testing.assert_allclose(dec, np.exp(-gamma * ((Xt[:, None, :] - sv[None]) ** 2).sum(-1)).dot(coef) + intercept,
                               rtol=0, atol=1e-9 * np.sum(np.abs(coef)))
    assert np.max(np.abs(dec - rdec)) <= b["decision"]
    outside = np.abs(rdec) > b["decision"]
    assert np.count_nonzero(~outside) <= 0.01 * M_TEST
    assert np.array_equal(svm.predict(Xt), dec > 0.0)
    assert np.array_equal(svm.predict(Xt)[outside], ref.predict(Xt)[outside])
    assert np.array_equal(svm.predict(X), finite)                  # the reference's assertion, through this trainer
    assert np.array_equal(ref.predict(Xt), ref._svc.predict(Xt).astype(bool))


def test_svm_class_pickles_arrays_only():
    dev = NumpyDevice()
    svm, X, _ = _trained("device", device=dev)
    blob = pickle.dumps(svm)
    assert b"NumpyDevice" not in blob and b"sklearn" not in blob
    back = pickle.loads(blob)
    assert back._dev is None and back.trainer == "device" and back.fit_info == svm.fit_info
    Xt = sn.probe_points(X, 200, seed=8)
    assert np.array_equal(back.decision_function(Xt), svm.decision_function(Xt))
    for a, b in zip(back.device_params(), svm.device_params()):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="bind"):
        back.fit(X, svm.y_train, 10.0)


def test_svm_class_falls_back_to_libsvm():
    # the iteration budget runs out (status 1)
    dev = NumpyDevice()
    svm, X, finite = _trained("device", device=dev, max_iter=10)
    ref, _, _ = _trained("libsvm", max_iter=10)
    assert dev.n_svm_fit == 1 and svm.fit_info["trainer_used"] == "libsvm" and svm.fit_info["status"] == 1
    assert "budget" in svm.fit_info["fallback"] and svm._fit is None
    for a, b in zip(svm.device_params(), ref.device_params()):
        assert np.array_equal(a, b)
    # spellings the device does not serve
    for kw in (dict(gamma="auto"), dict(kernel="poly"), dict(class_weight="balanced")):
        dev = NumpyDevice()
        svm, X, finite = _trained("device", device=dev, tol=1e-3, **kw)
        assert dev.n_svm_fit == 0 and svm.fit_info["trainer_used"] == "libsvm" and svm._svc is not None
        assert np.array_equal(svm.decision_function(X[:5]), svm._svc.decision_function(X[:5]))
    # N > 8192 (two well separated blobs: libsvm is done at once)
    rng = np.random.default_rng(3)
    Xb = np.concatenate([rng.normal(0.0, 0.05, (4100, 2)), rng.normal(1.0, 0.05, (4100, 2))])
    fb = np.arange(8200) < 4100
    dev = NumpyDevice()
    svm = SVM(trainer="device", tol=1e-3).bind(dev)
    svm.fit(Xb, _targets(Xb, fb), 10.0)
    assert dev.n_svm_fit == 0 and svm.fit_info["trainer_used"] == "libsvm" and "8192" in svm.fit_info["fallback"]
    # a numeric gamma is served
    dev = NumpyDevice()
    svm, _, _ = _trained("device", device=dev, tol=1e-3, gamma=2.5)
    assert dev.n_svm_fit == 1 and svm.fit_info["trainer_used"] == "device" and svm.device_params()[2] == 2.5
    with pytest.raises(ValueError, match="trainer"):
        SVM(trainer="gpu")


def test_default_trainer_is_libsvm_and_needs_no_device():
    svm, X, finite = _trained("libsvm", tol=1e-3)
    assert SVM().trainer == "libsvm" and not SVM().wants_device and svm._fit is None and svm._svc is not None
    assert svm.fit_info["trainer_used"] == "libsvm"


def test_gpr_trains_its_classifier_through_its_own_device():
    d, N = 3, 300
    model = sw.Model(d, sw.M52, N, seed=9)
    y = model.y.copy()
    y[model.X[:, 0] > 1.5] = -np.inf
    kw = dict(inf_threshold="20s", random_state=1)
    dev = NumpyDevice()
    gpr = sw.mirror(model.bounds, model.kid, model.theta, device=dev, account_for_inf=SVM(trainer="device", tol=EPS), **kw)
    twin = sw.mirror(model.bounds, model.kid, model.theta, device=NumpyDevice(), account_for_inf=SVM(tol=EPS), **kw)
    for g in (gpr, twin):
        g.append_to_data(model.X, y, fit_gpr=False)           # holds the reference's assertion on the labels of fit
    clf, ref = gpr.infinities_classifier, twin.infinities_classifier
    assert dev.n_svm_fit == 1 and clf._dev is dev and clf.fit_info["trainer_used"] == "device"
    assert ref.fit_info["trainer_used"] == "libsvm" and twin.device.n_svm_fit == 0
    assert np.array_equal(clf.y_finite, ref.y_finite) and len(gpr.X_train) == len(twin.X_train) < N
    Xc = np.random.default_rng(4).uniform(model.bounds[:, 0], model.bounds[:, 1], (M_TEST, d))
    X_ = gpr.preprocessing_X.transform(Xc)
    b = sn.bounds(np.abs(clf.device_params()[1]), np.abs(ref.device_params()[1]), EPS, d, clf.fit_info["n_iter"])
    rdec = ref.decision_function(X_)
    outside = np.abs(rdec) > b["decision"]
    assert np.count_nonzero(~outside) <= 0.01 * M_TEST
    m, mt = gpr.predict(Xc), twin.predict(Xc)
    assert np.array_equal(np.isneginf(m)[outside], np.isneginf(mt)[outside]) and np.isneginf(m).any() and np.isfinite(m).any()
    # a second append refits through the same device; a copy trains through its own
    gpr.append_to_data(Xc[:4], np.array([-1.0, -np.inf, -2.0, -3.0]), fit_gpr=False)
    assert dev.n_svm_fit == 2
