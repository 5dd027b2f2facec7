"""numpy stand-in for the device call of gpry_amd/maximize.py's ``maximize_acq`` (``dev.maximize_acq``, kernel in
gpry_amd/csrc/maximize_acq.hip) and the table of cases the walk tests run (tests/test_maximize_acq_cpu.py,
tests/test_maximize_acq_gpu.py).  The ascent, the replay, its margins, tolerances and left-out caps are those of
tests/tools/maximize_numpy.py, which this module imports and does not change.

``AcqNumpyDevice(ref, mean=None)``: value and exact gradient of the LogExp acquisition
a(x) = 2 zeta (y(x) - baseline) + log sqrt(sigma(x)^2 - sigma_n^2) from the float64 oracle ``ref`` (an ``OracleGPR``):
y from ``mean`` (``sampler_walk.Model.mean_fn``: the oracle's unclipped mean, -inf where the mirror's gates reject;
default: the oracle's own) clipped as ``predict`` clips it, sigma from ``_std_from_ktrans``, and with
G = ``kernel_gradient_x`` (N, d), w = V^T V k* (= K^-1 k*):

    d a / d x_k = (2 zeta y_std (G^T alpha_)_k - y_std^2 (G^T w)_k / (sigma^2 - sigma_n^2)) / x_span_k

(x_span: the span of the x-affine map, 1 without one) -- the gradient of the value, which is what the device climbs
with, NOT the reference's ``std_grad / (std - sigma_n) + 2 zeta mu_grad``.  a is -inf unless y is finite,
y > minus_inf_value and sigma^2 - sigma_n^2 > 0.  ``maximize_acq`` has the signature and the outputs of
``gpry_amd._lib.Device.maximize_acq``; the ascent is inherited from ``MaxNumpyDevice``: the same decisions as the device,
not the same bits.  (sigma under the classifier's verdict is not zeroed here as the device does: such a point has
y = -inf and a = -inf either way.)

``AcqWalk(name)``: the inputs of one ``maximize_acq`` call of a case, built like ``maximize_numpy.Walk`` from the oracle
alone.  Starts: N_STARTS uniform points of the box with a finite acquisition (training rows are no starts here:
sigma^2 - sigma_n^2 <= 0 on them).  H0: diag((l_k / (hi_k - lo_k))^2), maximize_acq's default, times the case's h0_scale.
The models, boxes, length scales and gtol of the table are chosen so that the stand-in's own trace on the oracle stays
within LEFT_OUT_CASE / LEFT_OUT_TABLE and runs enough steps (tests/test_maximize_acq_cpu.py asserts it)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maximize_numpy as mn  # noqa: E402

MAX_ITER, N_STARTS, MAX_HALVINGS = mn.MAX_ITER, mn.N_STARTS, mn.MAX_HALVINGS


class AcqNumpyDevice(mn.MaxNumpyDevice):
    def __init__(self, ref, mean=None):
        from oracle import gpry_oracle as orc
        self.orc, self.ref = orc, ref
        self.xspan = (ref.pre_X.hi - ref.pre_X.lo) if hasattr(ref.pre_X, "hi") else np.ones(ref.d)
        self.y_std = float(ref.pre_y.inverse_transform_scale(1.0))
        self.mean = mean
        super().__init__(None, None)

    def _ktrans(self, X):
        X_ = self.ref.pre_X.transform(np.atleast_2d(X))
        return X_, self.orc.kernel_matrix(X_, self.ref.theta, self.ref.kernel_id, Y=self.ref.X_train_)

    def y_sigma(self, X):
        """(y, sigma) as ``predict(X, return_std=True)`` gives them, y through ``mean`` where one was given."""
        ref = self.ref
        X = np.atleast_2d(np.asarray(X, dtype=float))
        X_, K = self._ktrans(X)
        y = ref.pre_y.inverse_transform(K.dot(ref.alpha_)) if self.mean is None else np.asarray(self.mean(X), dtype=float)
        if ref.clip_factor is not None:
            y = np.minimum(y, ref.clip_hi())
        return y, ref._std_from_ktrans(K, X_)

    def acq(self, X, zeta, baseline, sigma_n, minus_inf_value=-np.inf):
        y, sd = self.y_sigma(X)
        dv = sd ** 2 - sigma_n ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            a = 2 * zeta * (y - baseline) + np.log(np.sqrt(np.maximum(dv, 0.0)))
            ok = np.isfinite(y) & (y > minus_inf_value) & (dv > 0)
        return np.where(ok, a, -np.inf)

    def acq_grad_x(self, X, zeta, sigma_n):
        """The raw-coordinate gradient of ``acq`` (of the unclipped, ungated mean, as the device's)."""
        ref, orc = self.ref, self.orc
        X = np.atleast_2d(np.asarray(X, dtype=float))
        X_, K = self._ktrans(X)
        sd = ref._std_from_ktrans(K, X_)
        W = ref.V_.T.dot(ref.V_.dot(K.T))                      # (N, m): K^-1 k*
        out = np.empty(X.shape)
        for p, x_ in enumerate(X_):
            G = orc.kernel_gradient_x(x_, ref.X_train_, ref.theta, ref.kernel_id)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[p] = (2 * zeta * self.y_std * G.T.dot(ref.alpha_)
                          - self.y_std ** 2 * G.T.dot(W[:, p]) / (sd[p] ** 2 - sigma_n ** 2)) / self.xspan
        return out

    def maximize_acq(self, lo, hi, X0, fixed, H0, zeta, baseline, sigma_n, max_iter, max_halvings, gtol, ftol,
                     minus_inf_value, hooks=False, dtype=np.float64):
        if not (np.isfinite(sigma_n) and sigma_n >= 0) or not (np.isfinite(zeta) and np.isfinite(baseline)):
            raise ValueError(f"zeta = {zeta}, baseline = {baseline}, sigma_n = {sigma_n}")
        self.loglike = lambda X: self.acq(X, zeta, baseline, sigma_n, minus_inf_value)
        self.grad_x = lambda X: self.acq_grad_x(X, zeta, sigma_n)
        X0 = np.atleast_2d(np.asarray(X0, dtype=float))
        out = self.maximize_mean(lo, hi, X0, np.full(len(X0), np.nan), fixed, H0, max_iter, max_halvings, gtol, ftol,
                                 -np.inf, hooks=hooks, dtype=dtype)
        out["a"] = out.pop("y")
        if hooks:
            out["a_tr"] = out.pop("y_tr")
        out["y"], out["sigma"] = self.y_sigma(out["X"])
        return out


def as_mean_trace(out):
    """A ``maximize_acq`` result with the key names ``maximize_numpy.replay`` reads (y_tr for a_tr)."""
    tr = dict(out)
    tr["y_tr"] = tr["a_tr"]
    return tr


# ---- the walk table -------------------------------------------------------------------------------------------------
def _cases():
    import sampler_walk as sw
    c = {}
    # (ls: the kernel's length scales in unit-cube coordinates of the model's box, where sampler_walk's 0.3 leaves the
    # acquisition without structure in that dimension -- sigma^2 <= sigma_n^2 everywhere in d = 1, the prior between the
    # training rows in d >= 9 -- or, d = 3, gives inverse Hessians so ill-conditioned that the float64 replay differs from
    # the long double one by more than EPS_M)
    c["d=1 RBF N=70"] = dict(model=dict(d=1, kid=sw.RBF, N=70, affine=True), ls=0.03)
    c["d=1 RBF N=70 full step onto a training row"] = dict(model=dict(d=1, kid=sw.RBF, N=70, affine=False), ls=0.03, land=True)
    c["d=3 M52 N=300 one fixed"] = dict(model=dict(d=3, kid=sw.M52, N=300, affine=False), fixed=[1], ls=0.15)
    c["d=5 M12 N=70 two fixed"] = dict(model=dict(d=5, kid=sw.M12, N=70, affine=True), fixed=[0, 3], ls=0.6)
    c["d=9 M32 N=1100"] = dict(model=dict(d=9, kid=sw.M32, N=1100, affine=False), ls=0.8)
    c["d=17 RBF N=300"] = dict(model=dict(d=17, kid=sw.RBF, N=300, affine=True), ls=1.2)
    c["d=32 M52 N=1100"] = dict(model=dict(d=32, kid=sw.M52, N=1100, affine=False), ls=1.5)
    # the box's walls cut the way up the mean (its peak is at 0.3) off: the free set shrinks on the way and H is reset
    c["wall cuts the optimum off"] = dict(model=dict(d=3, kid=sw.M52, N=300, affine=True), hi={0: -0.2, 2: 0.1})
    # SVM + trust region (tests/test_nested_gpu.py: _svm_model): a long first step lands on gated ground
    c["gated"] = dict(model=dict(d=3, kid=sw.M52, N=300, svm=True, seed=9), ls=0.15, h0_scale=2.0)
    return c


class AcqWalk:
    """See the module's docstring.  Model: that of ``maximize_numpy.Walk`` (normalize_y off, noise 0.1); zeta =
    LogExp's d^-0.85, sigma_n = the noise level 0.1, baseline = the largest training value.

    The case ``land``: d = 1, and H0 = [[h]] with h = (u_T - u_0) / g(u_0) for start 0 and T the nearest training row
    uphill of it at least 0.02 of the box away -- the first full step of start 0 lands on T, where sigma^2 <= sigma_n^2
    and a = -inf, and is halved away."""

    def __init__(self, name, gpr_device=None):
        import sampler_walk as sw
        case = _cases()[name]
        margs = dict(case["model"])
        d = margs["d"]
        self.name = name
        self.model = m = sw.Model(normalize_y=False, noise_level=0.1, s=0.5 * np.sqrt(d), **margs)
        span_m = m.bounds[:, 1] - m.bounds[:, 0]
        if "ls" in case:
            m.theta = np.log(np.concatenate([[4.0], case["ls"] * (np.ones(d) if m.affine else span_m)]))
        self.gpr = m.gpr(device=gpr_device) if (m.svm or gpr_device is None) else None
        self.ref = m.oracle(self.gpr)
        self.dev = AcqNumpyDevice(self.ref, m.mean_fn(self.ref, self.gpr))
        self.zeta, self.sigma_n = float(d) ** -0.85, 0.1
        self.baseline = float(np.max(self.ref.y_train))
        self.lo, self.hi = m.bounds[:, 0].copy(), m.bounds[:, 1].copy()
        for k, v in case.get("hi", {}).items():
            self.hi[k] = v
        span = self.hi - self.lo
        rng = np.random.default_rng(11 + d)
        X = rng.uniform(self.lo, self.hi, (8 * N_STARTS, d))
        X = X[np.isfinite(self.value_of(X))]
        self.X0 = np.ascontiguousarray(X[:N_STARTS])
        assert len(self.X0) == N_STARTS, (name, len(self.X0))
        self.fixed = np.zeros(d, bool)
        self.fixed[case.get("fixed", [])] = True
        ls_raw = np.exp(m.theta[1:]) * (span_m if m.affine else 1.0)
        self.H0 = case.get("h0_scale", 1.0) * np.diag((ls_raw / span) ** 2)
        self.target = None
        if case.get("land"):
            u0 = (self.X0[0, 0] - self.lo[0]) / span[0]
            g0 = float(self.dev.acq_grad_x(self.X0[:1], self.zeta, self.sigma_n)[0, 0] * span[0])
            uT = (self.ref.X_train[:, 0] - self.lo[0]) / span[0]
            side = uT[(uT - u0) * np.sign(g0) >= 0.02]
            self.target = float(side[np.argmin(np.abs(side - u0))])
            self.H0 = np.array([[(self.target - u0) / g0]])
        self.gtol, self.ftol, self.minus_inf_value = case.get("gtol", 1e-3), 0.0, -np.inf

    def value_of(self, X):
        return self.dev.acq(X, self.zeta, self.baseline, self.sigma_n)

    def args(self):
        return (self.lo, self.hi, self.X0, self.fixed, self.H0, self.zeta, self.baseline, self.sigma_n, MAX_ITER,
                MAX_HALVINGS, self.gtol, self.ftol, self.minus_inf_value)

    def trace(self):
        """The oracle-side trace: ``AcqNumpyDevice`` with the hooks."""
        return self.dev.maximize_acq(*self.args(), hooks=True)

    def replay(self, trace, value_of=None, dtype=np.float64):
        return mn.replay(as_mean_trace(trace), self.lo, self.hi, self.X0, self.fixed, self.H0, MAX_ITER, MAX_HALVINGS,
                         self.gtol, self.ftol, -np.inf, value_of if value_of is not None else self.value_of, dtype)


ACQ_CASES = list(_cases())


# ---- the models of the value-and-gradient tests ---------------------------------------------------------------------
# the kernel's length scales in unit-cube coordinates of the model's box, per dimension: short enough that sigma^2 stays
# above the floor 0.01 C of the gradient comparison at more than half of the uniform points for every N <= 1100, long
# enough that the training set shapes sigma (measured on the oracle; the GPU test asserts the share)
VALUE_LS = {2: 0.03, 3: 0.1, 5: 0.2, 9: 0.45, 17: 1.0}


def value_model(d, kid, N, affine, seed=None):
    """``sampler_walk.Model`` with normalize_y off (y_std = 1) and noise 0.1.  y_std = 1 because the std_grad of
    ``gpr.predict``, which the comparison is set against, carries y_std twice as the reference's does
    (gpry/gpr.py:1236-1266) while d sigma / dx has it once."""
    import sampler_walk as sw
    m = sw.Model(d, kid, N, affine=affine, normalize_y=False, noise_level=0.1, seed=N + d if seed is None else seed)
    span = m.bounds[:, 1] - m.bounds[:, 0]
    m.theta = np.log(np.concatenate([[4.0], VALUE_LS[d] * (np.ones(d) if affine else span)]))
    return m


def host_gradient(gpr, X, lo, hi, zeta, sigma_n, affine_span):
    """(ref (m, d), std (m,)) from ``gpr.predict(x[None], return_std=True, return_mean_grad=True, return_std_grad=True)``:
    ref = s (2 zeta mu_grad + std std_grad / (std^2 - sigma_n^2)), s = (hi - lo) / span of the x-affine map."""
    ref, sd = np.empty(X.shape), np.empty(len(X))
    s = (np.asarray(hi) - np.asarray(lo)) / affine_span
    for p, x in enumerate(X):
        _, std, mg, sg = gpr.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True)
        sd[p] = std[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            ref[p] = s * (2 * zeta * np.ravel(mg) + std[0] * np.ravel(sg) / (std[0] ** 2 - sigma_n ** 2))
    return ref, sd


# ---- the host code on a stand-in ------------------------------------------------------------------------------------
class AcqHostGpr(mn.HostGpr):
    """What ``maximize_acq`` and ``BatchOptimizer(acq_optimizer="device")`` need of a regressor, around a stand-in."""

    def __init__(self, device, X, y, bounds, noise_level=0.1, minus_inf_value=-np.inf):
        super().__init__(device, X, y, bounds, minus_inf_value)
        self.noise_level, self.d = noise_level, np.asarray(bounds).shape[0]

    @property
    def y_max(self):
        return np.max(self.y_train)


def host_gpr_of(walk, noise_level=0.1):
    """The stand-in regressor of an ``AcqWalk``'s model: the oracle's training set around its ``AcqNumpyDevice``."""
    return AcqHostGpr(walk.dev, walk.ref.X_train, walk.ref.y_train, walk.model.bounds, noise_level)
