"""Finite / infinite classifier that gates GP predictions.

Same role and interface as ``gpry/svm.py`` (``fit`` :227, ``_is_finite_raw`` :273-295,
``is_finite`` :297, ``predict`` :308-347): an RBF support-vector classifier trained on
"y above (max - threshold)" labels.  Training is libsvm's through scikit-learn by default (``trainer="libsvm"``) or, on
request (``trainer="device"``), the same dual solved on the GPU by ``gpry_svm_fit`` (``Device.svm_fit``);
its decision function -- an RBF expansion over the support vectors -- is exported with
``device_params`` so that the NORA sweep evaluates it on the GPU for its 1e5-1e6 candidates
(``gpry_set_gates``), and ``GaussianProcessRegressor.predict`` lets the device apply it to its points as well
(option ``predict_gates``: the one-point calls of the samplers would otherwise spend 50-100 us in libsvm per call).

Unlike the reference this is not a subclass of ``sklearn.svm.SVC``: it owns one (``_svc``) only while the labels are
mixed, which are the only training sets libsvm has anything to learn from.  The public attributes GPry reads
(``y_finite``, ``all_finite``, ``at_least_one_finite``, ``diff_threshold``, ``abs_threshold``, ``n``, ``d``) are kept.
"""
import warnings

import numpy as np

from gpry_amd.tools import check_random_state

_UNTRAINED = "The SVM has not been trained yet."


class SVM:
    TRAINERS = ("libsvm", "device")
    DEVICE_MAX_N = 8192        # gpry_svm_fit's limit; larger sets go to libsvm

    def __init__(self, C=1e7, kernel="rbf", gamma="scale", tol=1e-3, random_state=None, trainer="libsvm", **svc_kwargs):
        if trainer not in self.TRAINERS:
            raise ValueError(f"trainer must be one of {self.TRAINERS}, got {trainer!r}")
        self.trainer = trainer
        self._svc_args = dict(C=C, kernel=kernel, gamma=gamma, tol=tol, **svc_kwargs)
        self.random_state = check_random_state(random_state, convert_to_random_state=True)
        self._svc = None
        self._dev = None           # the bound Device of trainer="device" (bind); never pickled
        self._fit = None           # a device fit: sv, coef, gamma, rho (arrays and floats only)
        self.fit_info = None
        self._fit_count = 0        # bumped by every fit: what the device-side copy of the decision function is keyed by
        self.X_train = self.y_train = self.y_finite = None
        self.diff_threshold = self._max_y = None
        self.at_least_one_finite = self.all_finite = False

    # -- the training set -------------------------------------------------------------------------
    n = property(lambda self: 0 if self.y_train is None else len(self.y_train), doc="number of training points")

    @property
    def d(self):
        if self.X_train is None:
            raise ValueError("You need to add some data before determining its dimension.")
        return self.X_train.shape[1]

    @property
    def abs_threshold(self):
        """Lowest target that still counts as finite."""
        return self._max_y - self.diff_threshold

    # -- labels -----------------------------------------------------------------------------------
    @staticmethod
    def _is_finite_raw(y, diff_threshold, max_y=None):
        """Threshold test (not a prediction).  ``isfinite`` matters for y = +inf with an infinite threshold and
        for NaN."""
        top = np.max(y) if max_y is None else max_y
        return np.greater_equal(y, top - diff_threshold) & np.isfinite(y)

    def is_finite(self, y):
        if self.y_train is None:
            raise ValueError("Cannot do anything: the SVM has not been trained yet!")
        return self._is_finite_raw(y, self.diff_threshold, self._max_y)

    # -- training ---------------------------------------------------------------------------------
    wants_device = property(lambda self: getattr(self, "trainer", "libsvm") == "device",
                            doc="the classifier trains through a bound Device (GaussianProcessRegressor binds its own)")

    def bind(self, device):
        """The Device that ``trainer="device"`` trains through (kept by reference; a pickle or copy drops it)."""
        self._dev = device
        return self

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_dev"] = None
        return state

    def _device_gamma(self, X):
        """gamma as a number where the device serves the spelling: a positive float, or "scale" computed as scikit-learn
        does, 1 / (d X.var()); None otherwise ("auto", a degenerate variance)."""
        gamma = self._svc_args["gamma"]
        if isinstance(gamma, str):
            if gamma != "scale":
                return None
            var = float(X.var())
            gamma = 1.0 / (X.shape[1] * var) if var > 0.0 else None
        try:
            gamma = None if gamma is None else float(gamma)
        except (TypeError, ValueError):
            return None
        return gamma if gamma is not None and np.isfinite(gamma) and gamma > 0.0 else None

    def _fit_device(self):
        """Train through the bound device; False (with the reason in ``fit_info``) where libsvm has to do it."""
        info = dict(trainer_used="libsvm", n_iter=None, status=None, objective=None, violation=None, device_ms=None,
                    fallback=None)
        self.fit_info = info
        args, X = self._svc_args, self.X_train
        gamma = self._device_gamma(X) if args["kernel"] == "rbf" else None
        extra = set(args) - {"C", "kernel", "gamma", "tol", "max_iter"}
        if self._dev is None:
            raise ValueError("SVM(trainer='device') needs a device: call bind(device) before fit.")
        if args["kernel"] != "rbf" or gamma is None or extra:
            info["fallback"] = "kernel, gamma or an SVC option that the device does not serve"
        elif len(X) > self.DEVICE_MAX_N:
            info["fallback"] = f"N = {len(X)} > {self.DEVICE_MAX_N}"
        if info["fallback"]:
            return False
        max_iter = args.get("max_iter", -1)
        res = self._dev.svm_fit(X, self.y_finite, args["C"], gamma, eps=args["tol"],
                                max_iter=None if max_iter is None or max_iter < 0 else max_iter)
        info.update({k: res[k] for k in ("n_iter", "status", "objective", "violation", "device_ms")})
        if res["status"] != 0:
            info["fallback"] = "the iteration budget ran out"
            return False
        sv = np.flatnonzero(res["alpha"] > 0.0)
        sign = np.where(self.y_finite[sv], 1.0, -1.0)
        self._fit = dict(sv=np.ascontiguousarray(X[sv], dtype=float), coef=sign * res["alpha"][sv], gamma=float(gamma),
                         rho=float(res["rho"]), support=sv)
        info["trainer_used"] = "device"
        return True

    def fit(self, X, y, diff_threshold):
        """Label the targets against ``max(y) - diff_threshold`` and train the classifier if both labels occur; returns
        the labels.  A training set of -inf only keeps the previous threshold (as the reference does)."""
        self._fit_count = getattr(self, "_fit_count", 0) + 1
        self.X_train, self.y_train = np.array(X, copy=True), np.array(y, copy=True)
        self.at_least_one_finite = not np.all(self.y_train == -np.inf)
        if not self.at_least_one_finite:
            self.y_finite = np.zeros(len(X), dtype=bool)
            return self.y_finite
        self.diff_threshold, self._max_y = diff_threshold, max(self.y_train)
        self.y_finite = self._is_finite_raw(self.y_train, diff_threshold, max_y=self._max_y)
        self.all_finite = bool(self.y_finite.all())
        self._fit, self.fit_info = None, None
        if not self.all_finite:
            if self.wants_device and self._fit_device():
                self._svc = None
                return self.y_finite
            from sklearn.svm import SVC
            self._svc = SVC(random_state=self.random_state, **self._svc_args).fit(self.X_train, self.y_finite)
            if self.fit_info is None:
                self.fit_info = dict(trainer_used="libsvm", n_iter=int(np.max(self._svc.n_iter_)), status=int(self._svc.fit_status_),
                                     objective=None, violation=None, device_ms=None, fallback=None)
        return self.y_finite

    def _has_decision_function(self):
        return (self.y_train is not None and self.at_least_one_finite and not self.all_finite
                and (self._svc is not None or getattr(self, "_fit", None) is not None))

    def device_params(self):
        """``(support_vectors, dual_coef, gamma, intercept, positive_is_finite)`` of the fitted
        two-class RBF SVC, with ``predict(x) == (sum_i coef_i exp(-gamma |x - sv_i|^2) + intercept
        > 0) == positive_is_finite``; ``None`` when there is nothing to evaluate on the device
        (not trained, all points finite or none, other kernel)."""
        svc = self._svc
        if not self._has_decision_function():
            return None
        fit = getattr(self, "_fit", None)
        if fit is not None:        # trained on the device: coef = y alpha over alpha > 0, intercept = -rho, +1 is "finite"
            return fit["sv"], np.ascontiguousarray(fit["coef"], dtype=float), fit["gamma"], -fit["rho"], True
        if svc.kernel != "rbf" or len(svc.classes_) != 2:
            return None
        as_f64 = lambda a: np.ascontiguousarray(a, dtype=float)     # noqa: E731
        return (as_f64(svc.support_vectors_), as_f64(svc.dual_coef_[0]), float(svc._gamma),
                float(svc.intercept_[0]), bool(svc.classes_[1]))

    # -- prediction -------------------------------------------------------------------------------
    def decision_function(self, X, chunk=4096):
        """Decision values of the trained classifier (positive: finite), whichever trainer made it."""
        if not self._has_decision_function():
            raise ValueError(_UNTRAINED if self.y_train is None else "The SVM has a single class: no decision function.")
        X = np.atleast_2d(np.asarray(X, dtype=float))
        fit = getattr(self, "_fit", None)
        if fit is None:
            return self._svc.decision_function(X)
        sv, coef, out = fit["sv"], fit["coef"], np.empty(len(X))
        sv2 = np.einsum("ij,ij->i", sv, sv)
        for s in range(0, len(X), chunk):
            x = X[s:s + chunk]
            r2 = np.maximum(np.einsum("ij,ij->i", x, x)[:, None] + sv2[None, :] - 2.0 * x.dot(sv.T), 0.0)
            out[s:s + chunk] = np.exp(-fit["gamma"] * r2).dot(coef) - fit["rho"]
        return out

    def predict(self, X, validate=True):
        """True where a finite target is expected.  (``validate`` is accepted for the reference's signature; the
        input always goes through ``atleast_2d``.)"""
        if self.y_train is None:
            raise ValueError(_UNTRAINED)
        X = np.atleast_2d(X)
        if self.all_finite or not self.at_least_one_finite:
            if not self.all_finite:
                warnings.warn("Only -inf points added to the classifier so far. Returning False unconditionally.")
            return np.full(len(X), bool(self.all_finite))
        return self.decision_function(X) > 0.0       # (libsvm's own verdict for two classes: its label 1 is True)
