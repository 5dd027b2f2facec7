"""State-interaction harness of one ``gpry_ctx``: no call may change another's answer.

A context is one long-lived object that every entry point reads and writes (the prediction factor, the objective's
scratch factor and its adoption cache, training coordinates left scaled for another theta, the resident candidate pool,
the Kriging-believer session, the resident predict kernel, cached norms, capacities, scratch arenas).  The rule this
module lets a test enforce: on one context no entry point changes the answer of any other, and a context that has held
other models answers like a fresh one.

* ``OPS``: the op table.  An op is a name, a callable ``op(dev, case) -> tuple of ndarrays / scalars`` whose inputs depend
  on the case alone (every op draws from its own generator, seeded by the case's input seed and the op's name; nothing is
  shared and no input array is handed out twice), the ``Device`` methods it needs, and ``model_neutral`` -- it leaves the
  model (training set, theta, maps, gates, options) as it found it.  ``table(dev)`` is the part of it that ``dev`` can
  run, padded with ``sync`` to an even length.
* ``sequences(n)``: n orderings of n ops that hold every ordered pair (A immediately before B) exactly once.
* ``build(dev, case)``: the canonical, shortest construction of a model.
* ``compare(got, want, where)``: equality of bits.

Used by tests/test_ctx_state_gpu.py (the library) and tests/test_ctx_state_cpu.py (the harness itself, against the
stateless test double).
"""
import inspect
import zlib

import numpy as np

from oracle import gpry_oracle as orc

MASK_CLASSIFIED_INF, MASK_OUTSIDE_TRUST = 1, 2
TILE = 128          # csrc/common.h: GPRY_TILE, the padding quantum of N (ctx.hip: ensure_capacity)


def padded(N):
    return -(-max(N, 1) // TILE) * TILE


# ---- models ---------------------------------------------------------------------------------------------------------
def box(d):
    """The raw box of every case of dimension d (a function of d alone: cases of one width share their op inputs)."""
    k = np.arange(d)
    return -1.0 - 0.1 * k, 2.0 + 0.05 * k


class Case:
    """One model: training set in model coordinates, theta, maps, gates, and the rows appended after the factorisation."""

    def __init__(self, name, N, d, kid, seed, xmap=True, ymap=True, clip=False, gates=False, scale=0.4, noise=1e-4,
                 input_seed=None):
        self.name, self.d, self.kid, self.seed = name, d, kid, seed
        self.input_seed = d if input_seed is None else input_seed
        rng = np.random.default_rng([seed, N, d])
        self.lo, self.hi = box(d)
        span = self.hi - self.lo
        X = self.lo + span * rng.uniform(size=(N, d))
        c = self.lo + span * (0.35 + 0.3 * rng.uniform(size=d))
        y = -0.5 * (((X - c) / (0.5 * span)) ** 2).sum(1) * 6.0 + 0.3 * np.sin(3.0 * (X / span).sum(1))
        self.y_mean, self.y_std = (float(y.mean()), float(y.std()) if N > 1 else 1.0) if ymap else (0.0, 1.0)
        self.X_ = (X - self.lo) / span if xmap else X
        self.y_ = (y - self.y_mean) / self.y_std
        self.alpha = np.full(N, noise)
        l = scale * (1.0 + 0.1 * np.arange(d)) * (1.0 if xmap else span.mean())
        self.theta = np.log(np.concatenate(([2.0], l)))
        self.affine = dict(x_lo=self.lo if xmap else None, x_span=span if xmap else None, y_mean=self.y_mean,
                           y_std=self.y_std, clip_hi=float(np.quantile(y, 0.9)) if clip else np.inf)
        self.gates = None
        if gates:
            sv = rng.uniform(size=(4, d)) if xmap else self.lo + span * rng.uniform(size=(4, d))
            self.gates = dict(sv=sv, coef=np.array([1.0, -0.8, 0.6, -0.7]), gamma=2.0 / (d if xmap else d * span.mean() ** 2),
                              intercept=0.15, positive_is_finite=True,
                              trust_bounds=np.column_stack([self.lo + 0.01 * span, self.hi - 0.005 * span]))
        self.appends = []
        self.baseline = float(y.max())
        self.zeta = float(d) ** -0.85

    @property
    def sigma_n(self):
        return float(np.sqrt(self.alpha[0])) * self.y_std

    def with_theta(self, shift, name):
        other = self.copy(name)
        other.theta = self.theta + shift
        return other

    def copy(self, name):
        other = Case.__new__(Case)
        other.__dict__.update(self.__dict__)
        other.name, other.appends, other.affine = name, list(self.appends), dict(self.affine)
        return other

    def appended(self, k, name):
        """This case followed by ``append_rows`` of k further rows of the same function."""
        other = self.copy(name)
        rng = np.random.default_rng([self.seed, 77, len(self.appends), k])
        span = self.hi - self.lo
        Xn = rng.uniform(size=(k, self.d))
        xmap = self.affine["x_lo"] is not None
        raw = self.lo + span * Xn
        yn = -0.5 * (((raw - self.lo - 0.5 * span) / (0.5 * span)) ** 2).sum(1) * 6.0
        other.appends.append((Xn if xmap else raw, (yn - self.y_mean) / self.y_std, np.full(k, self.alpha[0])))
        return other

    # -- fixed inputs of the ops -------------------------------------------------------------------------------------
    def rng(self, tag):
        return np.random.default_rng([self.input_seed, zlib.crc32(tag.encode())])

    def points(self, tag, m, margin=0.0):
        """m raw points of the box (margin > 0: a little beyond it, where the trust box gates them)."""
        u = self.rng(tag).uniform(-margin, 1.0 + margin, size=(m, self.d))
        return self.lo + (self.hi - self.lo) * u

    def theta_other(self, k=1):
        return self.theta + 0.07 * k * np.cos(np.arange(self.d + 1) + k)

    def theta_nonpd(self):
        """The construction of the goldens' f3_nonpd (duplicated rows, no noise, huge length scale) reached through theta
        alone: length scales of 1e30 make every row of K the same row, and an amplitude of 1e20 puts the noise below
        half an ulp of the diagonal -- K is C times the matrix of ones, whose second or third pivot is not positive."""
        return np.log(np.concatenate(([1e20], np.full(self.d, 1e30))))


def build(dev, case):
    """The canonical, shortest construction of ``case`` on ``dev``."""
    dev.set_train(case.X_, case.y_, case.alpha)
    dev.set_theta(case.kid, case.theta)
    dev.set_affine(**case.affine)
    dev.set_gates(**(case.gates or {}))
    info = dev.factorize()
    assert info == 0, f"{case.name}: factorize reports {info}"
    for Xn, yn, an in case.appends:
        info = dev.append_rows(Xn, yn, an)
        assert info == 0, f"{case.name}: append_rows reports {info}"


# ---- results ----------------------------------------------------------------------------------------------------------
def flat(x):
    """An op's answer as a flat tuple of arrays: dicts in key order without their device times, records by field."""
    if x is None:
        return ()
    if isinstance(x, dict):
        return tuple(v for k in sorted(x) if k != "device_ms" for v in flat(x[k]))
    if isinstance(x, (tuple, list)):
        return tuple(v for item in x for v in flat(item))
    a = np.asarray(x)
    if a.dtype.names:
        return tuple(np.ascontiguousarray(a[f]) for f in a.dtype.names)
    return (a.copy(),)


def same_bits(a, b):
    """Exact equality, NaN in the same places (and with them +-inf: those compare as numbers)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))
    return bool(np.array_equal(a, b))


def difference(got, want):
    """None, or a line that says which output differs and by how much."""
    if len(got) != len(want):
        return f"{len(got)} outputs, expected {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        if not same_bits(a, b):
            a, b = np.asarray(a), np.asarray(b)
            if a.shape != b.shape or a.dtype != b.dtype:
                return f"output {i}: {a.dtype}{a.shape}, expected {b.dtype}{b.shape}"
            bad = np.flatnonzero(~((a == b) | ((a != a) & (b != b))).ravel())
            with np.errstate(all="ignore"):
                gap = np.abs(a.ravel()[bad].astype(float) - b.ravel()[bad].astype(float))
            worst = float(np.max(gap[np.isfinite(gap)])) if np.isfinite(gap).any() else np.nan
            return (f"output {i}: {len(bad)} of {a.size} entries differ, first at {bad[0]}: {a.ravel()[bad[0]]!r} != "
                    f"{b.ravel()[bad[0]]!r}, largest |difference| {worst:.3e}")
    return None


def where(case, before, name):
    return f"{case.name}: {' -> '.join(list(before) + [name])}: op {name!r}"


def compare(got, want, at):
    diff = difference(got, want)
    assert diff is None, f"{at} does not give the bits of a fresh context: {diff}"


# ---- the op table -------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, fn, needs=(), model_neutral=True):
        self.name, self.fn, self.needs, self.model_neutral = name, fn, tuple(needs), model_neutral

    def available(self, dev):
        """Every needed method is there ("method:keyword": and takes that keyword)."""
        for need in self.needs:
            method, _, keyword = need.partition(":")
            if not hasattr(dev, method) or (keyword and keyword not in inspect.signature(getattr(dev, method)).parameters):
                return False
        return True

    def __call__(self, dev, case):
        return flat(self.fn(dev, case))

    def __repr__(self):
        return self.name


OPS = []


def op(name, *needs):
    def register(fn):
        OPS.append(Op(name, fn, needs))
        return fn
    return register


class option:
    """An option set for the length of a ``with`` block and put back to what it was (the double has none: 0)."""

    def __init__(self, dev, **values):
        self.dev, self.values, self.old = dev, values, {}

    def __enter__(self):
        for k, v in self.values.items():
            self.old[k] = self.dev.get_option(k) if hasattr(self.dev, "get_option") else 0
            self.dev.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.dev.set_option(k, v)


def refused(call):
    """The call must raise; what it raises is not part of the answer."""
    try:
        call()
    except AssertionError:
        raise
    except Exception:           # noqa: BLE001 (ValueError from the binding, GpryHipError from the library)
        return (np.array(1),)
    raise AssertionError("a call that the ABI documents as refused was answered")


# -- the objective
@op("lml_other", "lml")
def _(dev, case):
    return dev.lml(case.theta_other(1), True), dev.lml(case.theta_other(1), False)


# (the three ops below stand in this order on purpose: the zigzag path that starts at lml_own goes on with kernel_train
# and then refactorize -- a borrower of the scratch factor between the evaluation that arms the adoption and the
# factorisation that adopts)
@op("refactorize", "get_factor")
def _(dev, case):
    assert not case.appends, "refactorize: a bordered factor and a factorisation of all rows differ by rounding"
    dev.set_theta(case.kid, case.theta)
    info = dev.factorize()
    return (info,) + tuple(dev.get_factor())


@op("lml_own", "lml")
def _(dev, case):
    return dev.lml(case.theta, True)


@op("kernel_train", "kernel_train")
def _(dev, case):
    return dev.kernel_train(add_alpha=True), dev.kernel_train(add_alpha=False)


@op("lml_nonpd", "lml")
def _(dev, case):
    return dev.lml(case.theta_nonpd(), True)


def _thetas(case):
    return np.array([case.theta_other(2), case.theta, case.theta_other(3)])


@op("lml_batch_latency", "lml_batch")
def _(dev, case):
    with option(dev, lml_schedule=0):
        return dev.lml_batch(_thetas(case), True)


@op("lml_batch_throughput", "lml_batch")
def _(dev, case):
    with option(dev, lml_schedule=1):
        return dev.lml_batch(_thetas(case), True)


# -- the evaluations at a theta that is not the model's own which came after gpry_lml: each borrows the scratch factor
@op("loo_objective", "loo_objective")
def _(dev, case):
    return dev.loo_objective(case.theta_other(1), True), dev.loo_objective(case.theta_other(1), False)


@op("loo_objective_nonpd", "loo_objective")
def _(dev, case):
    return dev.loo_objective(case.theta_nonpd(), True)


@op("loo_objective_batch", "loo_objective_batch")
def _(dev, case):
    return dev.loo_objective_batch(_thetas(case), True)


@op("lml_hessian", "lml_hessian")
def _(dev, case):
    return dev.lml_hessian(case.theta_other(1))


@op("kernel_cross", "kernel_cross")
def _(dev, case):
    u = case.rng("kernel_cross").uniform(size=(37, case.d))
    return dev.kernel_cross(u if case.affine["x_lo"] is not None else case.lo + (case.hi - case.lo) * u)


@op("get_factor", "get_factor")
def _(dev, case):
    return dev.get_factor()


# -- predict through each of its paths
@op("predict_1_served", "predict")
def _(dev, case):
    X = case.points("predict_1", 2)
    return dev.predict(X[:1]), dev.predict(X[1:])         # the second is answered by the kernel the first left running


@op("predict_1_launched", "predict")
def _(dev, case):
    X = case.points("predict_1", 2)
    with option(dev, predict_serve=0):
        return dev.predict(X[:1]), dev.predict(X[1:])


def _predict_std(tag, m):
    def fn(dev, case):
        return dev.predict(case.points(tag, m, margin=0.03), return_std=True)
    return fn


op("predict_5_std", "predict")(_predict_std("predict_5", 5))            # the <= 16 path
op("predict_17_std", "predict")(_predict_std("predict_17", 17))         # split-K
op("predict_130_std", "predict")(_predict_std("predict_130", 130))
op("predict_3000_std", "predict")(_predict_std("predict_3000", 3000))   # panel


@op("predict_masked", "predict")
def _(dev, case):
    X = case.points("predict_masked", 40)
    r = case.rng("predict_masked bits")
    mask = (r.uniform(size=40) < 0.25) * MASK_CLASSIFIED_INF | (r.uniform(size=40) < 0.25) * MASK_OUTSIDE_TRUST
    return dev.predict(X, return_std=True, mask=mask.astype(np.uint8)), dev.predict(X, mask=mask.astype(np.uint8))


@op("predict_grad", "predict_grad")
def _(dev, case):
    return dev.predict_grad(case.points("predict_grad", 1)[0], want_kinv=True, want_kgrad=True)


@op("predict_point", "predict_point")
def _(dev, case):
    return dev.predict_point(case.points("predict_point", 1)[0])


@op("predict_grad_batch_2", "predict_grad_batch")
def _(dev, case):
    return dev.predict_grad_batch(case.points("predict_grad_batch_2", 2), True)


@op("predict_grad_batch_130", "predict_grad_batch")
def _(dev, case):
    return dev.predict_grad_batch(case.points("predict_grad_batch_130", 130), True)


# -- the sweep of a pool of its own
SWEEP_M = 5003


def sweep_pool(case):
    return case.points("sweep pool", SWEEP_M, margin=0.02)


def _topk(dev):
    top, bound = dev.sweep_topk(40)
    return top, bound


@op("sweep", "sweep_logexp", "sweep_topk", "sweep_fetch")
def _(dev, case):
    with option(dev, sweep_chunk=1024):
        out = dev.sweep_logexp(sweep_pool(case), case.zeta, case.baseline, case.sigma_n)
        return out, _topk(dev), dev.sweep_fetch(("y", "sigma", "acq"))


@op("sweep_given_y", "sweep_logexp:y_given", "sweep_topk")
def _(dev, case):
    """The sampler's own y: only sigma is computed."""
    y = case.baseline - 5.0 * case.rng("given y").uniform(size=1500)
    with option(dev, sweep_chunk=1024):
        out = dev.sweep_logexp(case.points("given pool", 1500), case.zeta, case.baseline, case.sigma_n, y_given=y)
        return out, _topk(dev)


@op("sweep_pruned", "sweep_logexp", "sweep_topk")
def _(dev, case):
    with option(dev, sweep_chunk=1024, sweep_prune=1):
        out = dev.sweep_logexp(case.points("pruned pool", SWEEP_M, margin=0.02), case.zeta, case.baseline, case.sigma_n, want=())
        return out["n_nan"], _topk(dev)


# -- a Kriging-believer session
KB_ROWS = (40, 30)


def kb_points(case):
    return case.points("kb session", sum(KB_ROWS))


@op("kb_session", "kb_reset", "kb_register", "kb_gram", "kb_gram_rows")
def _(dev, case):
    X = kb_points(case)
    dev.kb_reset()
    a = dev.kb_register(X[:KB_ROWS[0]])
    b = dev.kb_register(X[KB_ROWS[0]:])
    n = sum(KB_ROWS)
    return a, b, dev.kb_gram(n - 1, n), dev.kb_gram(3, n), dev.kb_gram_rows([0, 41, n - 1, 7], n)


@op("kb_rank", "kb_reset", "kb_rank", "predict")
def _(dev, case):
    """The arguments of KBSession.rank / RankedPool._add_native (tests/tools/kb_rank_common.py drives those): a fresh
    session, the whole offer new to it, an empty pool of 3 points."""
    X = case.points("kb_rank", 24)
    y, sigma = dev.predict(X, return_std=True)
    acq = orc.logexp_f(y, sigma, case.baseline, case.sigma_n, case.zeta)
    keep = np.isfinite(acq)                         # (the native ranking is for models without a classifier: no -inf rows)
    X, y, sigma, acq = (np.ascontiguousarray(a[keep]) for a in (X, y, sigma, acq))
    m, n_points = len(X), 3
    var0 = np.empty(m)
    slots = (np.full(n_points + 1, -1, np.int64), np.zeros(n_points + 1), np.zeros(n_points + 1), np.zeros(n_points + 1),
             np.full(n_points + 1, -np.inf))
    order = np.ascontiguousarray(np.argsort(acq)[::-1], dtype=np.int64)
    dev.kb_reset()
    models, info, _ = dev.kb_rank(X, var0, np.arange(m, dtype=np.int64), y, sigma, acq, order,
                                  [case.sigma_n, float(case.alpha[0]), case.baseline, case.zeta, case.y_std], slots)
    return models, info, var0, slots


# -- derivatives, joint predictive, cross-validation
@op("hessian_mean", "hessian_mean")
def _(dev, case):
    return dev.hessian_mean(case.points("hessian_mean", 3))


@op("predict_cov", "predict_cov")
def _(dev, case):
    return dev.predict_cov(case.points("predict_cov", 33))


@op("sample_joint", "sample_joint")
def _(dev, case):
    return dev.sample_joint(case.points("sample_joint", 33), 4, 20240607)


@op("loo", "loo")
def _(dev, case):
    return dev.loo()


@op("leave_out", "leave_out")
def _(dev, case):
    r = case.rng("leave_out")
    return dev.leave_out([r.choice(dev.N, min(s, dev.N), replace=False) for s in (1, 16, 17)])


@op("predict_without", "predict_without")
def _(dev, case):
    r = case.rng("predict_without")
    return dev.predict_without([r.choice(dev.N, min(s, dev.N), replace=False) for s in (1, 3)],
                               case.points("predict_without", 37))


# -- derivatives in theta, and the predictive under a batch of thetas
@op("mean_theta_grad", "mean_theta_grad")
def _(dev, case):
    return dev.mean_theta_grad(case.points("mean_theta_grad", 37))


@op("var_theta_grad", "var_theta_grad")
def _(dev, case):
    return dev.var_theta_grad(case.points("var_theta_grad", 37))


def _predict_thetas(want_var):
    def fn(dev, case):
        thetas = np.array([case.theta_other(k) for k in (1, 2, 3)])
        return dev.predict_thetas(thetas, case.points("predict_thetas", 37), want_var=want_var)
    return fn


op("predict_thetas", "predict_thetas")(_predict_thetas(False))
op("predict_thetas_var", "predict_thetas:want_var")(_predict_thetas(True))


@op("svm_fit", "svm_fit")
def _(dev, case):
    X = case.rng("svm_fit").uniform(size=(65, case.d))
    s = X[:, 0] + 0.5 * X[:, -1]
    return dev.svm_fit(X, s < np.median(s) + 0.1, 10.0, 1.0 / (case.d * X.var()))


# -- the samplers
def _survivors(dev, case):
    X, y, _ = dev.ns_prior(case.lo, case.hi, 31, 96)
    order = np.argsort(y, kind="stable")
    return np.ascontiguousarray(X[order[32:]]), np.ascontiguousarray(y[order[32:]]), float(y[order[31]])


@op("ns_prior", "ns_prior")
def _(dev, case):
    return dev.ns_prior(case.lo, case.hi, 5, 48)[:2]


@op("ns_generation", "ns_prior", "ns_generation")
def _(dev, case):
    Xs, ys, lstar = _survivors(dev, case)
    W = 0.2 * np.eye(case.d)
    plain = dev.ns_generation(case.lo, case.hi, Xs, ys, lstar, W, 1, 0, 8, 4)[:3]
    # ... and with two clusters of survivors, their own matrices and prior volumes
    volumes = dev.ns_generation(case.lo, case.hi, Xs, ys, lstar, np.array([W, 0.5 * W]), 1, 0, 8, 4,
                                labels=np.arange(len(Xs), dtype=np.int32) % 2, cum_p=np.array([0.4, 1.0]))[:3]
    return plain, volumes


@op("ns_generation_phantoms", "ns_prior", "ns_generation_phantoms")
def _(dev, case):
    Xs, ys, lstar = _survivors(dev, case)
    return dev.ns_generation_phantoms(case.lo, case.hi, Xs, ys, lstar, 0.2 * np.eye(case.d), 1, 0, 8, 4, 1)[:5]


@op("ns_knn", "ns_knn")
def _(dev, case):
    return dev.ns_knn(case.lo, case.hi, case.points("ns_knn", 40), 4)[0]


def _starts(case, tag, n=8):
    u = 0.3 + 0.4 * case.rng(tag).uniform(size=(n, case.d))
    return case.lo + (case.hi - case.lo) * u


@op("mcmc_chains", "mcmc_chains")
def _(dev, case):
    return dev.mcmc_chains(case.lo, case.hi, _starts(case, "mcmc"), np.full(8, np.nan), 0.05 * np.eye(case.d), 1.0, -np.inf,
                           7, 1, 5, 1)


@op("mcmc_ladders", "mcmc_ladders")
def _(dev, case):
    Lp = np.array([s * np.eye(case.d) for s in (0.04, 0.1)])
    return dev.mcmc_ladders(case.lo, case.hi, _starts(case, "ladders"), np.full(8, np.nan), 2, Lp, [1.0, 3.0], -np.inf,
                            11, 2, 5, 1, 2)


def _hmc(reflect):
    def fn(dev, case):
        return dev.hmc_chains(case.lo, case.hi, _starts(case, "hmc"), np.full(8, np.nan), 0.3 * np.eye(case.d), 0.3, 4, 1.0,
                              -np.inf, 13, 0, 5, 1, reflect=reflect)
    return fn


op("hmc_chains", "hmc_chains")(_hmc(False))
op("hmc_chains_reflect", "hmc_chains")(_hmc(True))


@op("maximize_mean", "maximize_mean")
def _(dev, case):
    return dev.maximize_mean(case.lo, case.hi, _starts(case, "maximize", 4), np.full(4, np.nan), np.zeros(case.d, bool),
                             np.eye(case.d), 3, 12, 1e-6, 0.0, -np.inf)


@op("maximize_acq", "maximize_acq")
def _(dev, case):
    return dev.maximize_acq(case.lo, case.hi, _starts(case, "maximize_acq", 4), np.zeros(case.d, bool), np.eye(case.d),
                            case.zeta, case.baseline, case.sigma_n, 3, 12, 1e-6, 0.0, -np.inf)


@op("microbench", "microbench")
def _(dev, case):
    dev.microbench(1, 1 << 22)          # (a rate: what it returns is no answer to compare)
    return ()


# -- options that are set and set back within the op
@op("opt_gemm_dma", "set_option", "lml")
def _(dev, case):
    with option(dev, gemm_dma=0):
        return dev.lml(case.theta_other(4), True)


@op("opt_predict_small", "set_option", "predict")
def _(dev, case):
    with option(dev, predict_small=0):
        return dev.predict(case.points("opt_predict_small", 20))


@op("opt_sweep_upload", "set_option", "sweep_logexp", "sweep_topk")
def _(dev, case):
    with option(dev, sweep_upload=0, sweep_chunk=1024):
        return dev.sweep_logexp(case.points("opt_sweep_upload", 2051), case.zeta, case.baseline, case.sigma_n), _topk(dev)


@op("opt_cross_mfma", "set_option", "predict")
def _(dev, case):
    with option(dev, cross_mfma=0):
        return dev.predict(case.points("opt_cross_mfma", 3000), return_std=True)


# -- calls that the ABI refuses: each must raise, and leave everything else answering as before
@op("refused_predict_columns", "predict")
def _(dev, case):
    return refused(lambda: dev.predict(np.full((3, case.d + 1), 0.5), return_std=True))


@op("refused_leave_out_index", "leave_out")
def _(dev, case):
    return refused(lambda: dev.leave_out([[0, dev.N]]))


@op("refused_hmc_box", "hmc_chains")
def _(dev, case):
    return refused(lambda: dev.hmc_chains(case.lo, case.lo, _starts(case, "hmc"), np.full(8, np.nan), 0.3 * np.eye(case.d), 0.3,
                                          4, 1.0, -np.inf, 13, 0, 5, 1))


SYNC = Op("sync", lambda dev, case: dev.sync(), ("sync",))
assert len({o.name for o in OPS}) == len(OPS)

# what a transition test probes after every change of model: the three predict paths, the x-gradient, the objective, sweep
# and shortlist, a Kriging-believer session, Hessian, joint covariance, cross-validation, a Metropolis walk, an ascent
PROBES = ("predict_1_served", "predict_5_std", "predict_17_std", "predict_3000_std", "predict_grad", "lml_other", "sweep",
          "kb_session", "hessian_mean", "predict_cov", "loo", "mcmc_chains", "maximize_acq")
# ... and those of them that read the prediction factor: without a valid factor they must raise, not answer
PREDICTION_PROBES = tuple(p for p in PROBES if p != "lml_other")


def table(dev):
    """``(ops that dev can run, names of those it cannot)``; an odd table gains ``sync``."""
    ops = [o for o in OPS if o.available(dev)]
    if len(ops) % 2:
        ops.append(SYNC)
    return ops, [o.name for o in OPS if not o.available(dev)]


def by_name(ops, names):
    have = {o.name: o for o in ops}
    return [have[n] for n in names if n in have]


# ---- orderings ------------------------------------------------------------------------------------------------------
def sequences(n):
    """For even n, the n / 2 zigzag Hamiltonian paths k, k + 1, k - 1, k + 2, k - 2, ... (mod n), k = 0 .. n / 2 - 1, each
    forwards and backwards: n orderings of 0 .. n - 1 in which every ordered pair (a immediately before b), a != b,
    occurs exactly once (the paths are Walecki's decomposition of the complete graph on n vertices)."""
    if n % 2 or n < 2:
        raise ValueError("sequences: n must be even and at least 2")
    for k in range(n // 2):
        path = [k]
        for j in range(1, n // 2 + 1):
            path.append((k + j) % n)
            if len(path) < n:
                path.append((k - j) % n)
        yield path
        yield path[::-1]


# ---- runs -------------------------------------------------------------------------------------------------------------
def baselines(make_dev, case, ops, again=None):
    """Each op's answer on a context that has run ``build`` and nothing else: one fresh context per op.  ``again``: a dict
    that receives the op's answer from a second call on that context, straight after the first."""
    out = {}
    for o in ops:
        dev = make_dev()
        try:
            build(dev, case)
            out[o.name] = o(dev, case)
            if again is not None:
                again[o.name] = o(dev, case)
        finally:
            if hasattr(dev, "close"):
                dev.close()
    return out


def close_enough(got, want, rtol):
    """The fall-back comparison of an op that the code documents as not bit-repeatable."""
    return len(got) == len(want) and all(
        np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True) for a, b in zip(got, want))


def run_sequence(dev, case, ops, want, collect=None, tolerant=None):
    """Run ``ops`` in order on ``dev`` (which holds ``case``) and compare every answer with ``want[name]``.  ``collect``: a
    list that receives ``(previous op, op, message)`` of every mismatch instead of the first one being raised.
    ``tolerant``: {op name: rtol} of the ops that are compared to a tolerance instead of bit for bit."""
    done = []
    for o in ops:
        at = where(case, done, o.name)
        try:
            got = o(dev, case)
        except AssertionError:
            raise
        except Exception as e:          # noqa: BLE001
            raise AssertionError(f"{at} raised {type(e).__name__}: {e}") from e
        diff = difference(got, want[o.name])
        if diff is not None and tolerant and o.name in tolerant and close_enough(got, want[o.name], tolerant[o.name]):
            diff = None
        if diff is not None:
            msg = f"{at} does not give the bits of a fresh context: {diff}"
            if collect is None:
                raise AssertionError(msg)
            collect.append((done[-1] if done else None, o.name, msg))
        done.append(o.name)


def probe(dev, case, ops):
    """The answers of ``ops`` on ``dev``, a refusal noted as such (whoever compares two contexts wants the same refusals)."""
    out = {}
    for o in ops:
        try:
            out[o.name] = o(dev, case)
        except AssertionError:
            raise
        except Exception as e:          # noqa: BLE001
            out[o.name] = ("raised", type(e).__name__)
    return out


def compare_probes(got, want, case, history):
    for name in want:
        at = f"{case.name} after {' => '.join(history)}: probe {name!r}"
        g, w = got[name], want[name]
        if w and isinstance(w[0], str) or g and isinstance(g[0], str):
            assert g == w, f"{at}: {g} on the used context, {w} on a fresh one"
        else:
            compare(g, w, at)


# ---- the models of the tests ------------------------------------------------------------------------------------------
M52, M32, M12, RBF = 3, 2, 1, 0


def model_a(N=300):
    """The general objective chain with the adoption cache live; X map, clipping, device gates."""
    return Case(f"a (N={N}, d=5, Matern-5/2, X map, clip, gates)", N, 5, M52, seed=1, clip=True, gates=True)


def model_b(N=100):
    """The 32-wide dimension instantiation; no map, no gates.  (d > 16 keeps it off the single-launch objective although
    N <= 128: model c is the one that takes it.)"""
    return Case(f"b (N={N}, d=17, RBF, no map, no gates)", N, 17, RBF, seed=2, xmap=False, ymap=False, scale=1.0)


def model_c(N=100):
    """The single-launch objective (N <= 128, d <= 16): it leaves no factor to adopt and does not rescale the training
    coordinates, so what an evaluation leaves behind differs from models a and b."""
    return Case(f"c (N={N}, d=12, RBF, no map, no gates)", N, 12, RBF, seed=3, xmap=False, ymap=False, scale=1.0)


class Step:
    """One transition of the chain: ``case`` is the model it leads to, ``how(dev)`` the calls that make it on the
    long-lived context (None: ``build``), ``same_width``: d stays, so the resident candidate pool is still a pool of this
    model, ``keeps_factor``: no call of it touches the factor, so a Kriging-believer session stands."""

    def __init__(self, label, case, how=None, same_width=False, keeps_factor=False):
        self.label, self.case, self.how, self.same_width, self.keeps_factor = label, case, how, same_width, keeps_factor

    def apply(self, dev):
        if self.how is None:
            build(dev, self.case)
        else:
            self.how(dev)


def chain(sizes=(300, 100, 129, 128, 1, 1100), k_inside=3, k_past=90):
    """The chain of models one context goes through (the sizes are arguments so that the test of the harness itself can
    run a small one): 1 N=300 d=5 Matern-5/2; 2 the same data at another theta, reached through lml(theta), set_theta,
    factorize (adoption); 3 append_rows inside the padded size; 4 append_rows past it; 5 N=100 d=17 RBF (fewer, wider
    rows); 6 N=129 d=3 Matern-1/2 (narrower rows, just above the single-launch limit); 7 N=128 d=3; 8 N=1 d=1;
    9 N=1100 d=8 Matern-3/2 with gates; 10 the same with the gates off and another y map; 11 model 1 again."""
    n1, n5, n6, n7, n8, n9 = sizes
    c1 = Case(f"1 (N={n1}, d=5, Matern-5/2)", n1, 5, M52, seed=11)
    c2 = c1.with_theta(0.1 * np.cos(np.arange(6)), "2 (model 1 at another theta)")
    c3 = c2.appended(k_inside, f"3 (model 2 and {k_inside} appended rows)")
    c4 = c3.appended(k_past, f"4 (model 3 and {k_past} appended rows)")
    c5 = Case(f"5 (N={n5}, d=17, RBF, no map)", n5, 17, RBF, seed=12, xmap=False, scale=1.0)
    c6 = Case(f"6 (N={n6}, d=3, Matern-1/2)", n6, 3, M12, seed=13)
    c7 = Case(f"7 (N={n7}, d=3, Matern-1/2)", n7, 3, M12, seed=14)
    c8 = Case(f"8 (N={n8}, d=1, Matern-5/2)", n8, 1, M52, seed=15)
    c9 = Case(f"9 (N={n9}, d=8, Matern-3/2, gates)", n9, 8, M32, seed=16, gates=True)
    c10 = c9.copy("10 (model 9, gates off, another y map)")
    c10.gates = None
    c10.affine.update(y_mean=c9.y_mean + 0.5, y_std=1.5 * c9.y_std, clip_hi=c9.y_mean + 0.2 * c9.y_std)
    c10.y_mean, c10.y_std = c10.affine["y_mean"], c10.affine["y_std"]

    def adopt(dev):
        dev.lml(c2.theta, True)
        dev.set_theta(c2.kid, c2.theta)
        assert dev.factorize() == 0

    def append(case):
        def how(dev):
            assert dev.append_rows(*case.appends[-1]) == 0
        return how

    def regate(dev):
        dev.set_gates()
        dev.set_affine(**c10.affine)

    return [Step("build 1", c1), Step("lml, set_theta, factorize at the theta of 2", c2, adopt, same_width=True),
            Step(f"append {k_inside}", c3, append(c3), same_width=True), Step(f"append {k_past}", c4, append(c4), same_width=True),
            Step("build 5", c5), Step("build 6", c6), Step("build 7", c7, same_width=True), Step("build 8", c8),
            Step("build 9", c9), Step("set_gates(), set_affine of 10", c10, regate, same_width=True, keeps_factor=True),
            Step("build 1 again", c1)]


def failed_append_case():
    return Case("failed append (N=50, d=2, RBF)", 50, 2, RBF, seed=3)


def bad_border(case):
    """A copy of the first training row whose diagonal entry is pushed down: the Schur complement of the border is
    negative, ``append_rows`` reports the pivot and the context holds no valid factor any more."""
    return case.X_[:1].copy(), case.y_[:1].copy(), np.array([-0.5])
