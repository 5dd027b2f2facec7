"""ctypes binding of ``libgpry_hip.so`` (C ABI declared in ``include/gpry_hip.h``).

There is deliberately no CPU fallback: if the shared library is missing, or a device
call is made on a machine without a GPU, the error is raised to the caller.
"""
import ctypes as C
import ctypes as _ct     # for svm_fit, whose parameter C is the classifier's
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgpry_hip.so")

GPRY_MAX_DIM = 32      # include/gpry_hip.h: ABI array size and the enforced limit on d
MASK_CLASSIFIED_INF = 1
MASK_OUTSIDE_TRUST = 2

KERNEL_IDS = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}
KERNEL_WHITE = 0x10    # GPRY_KERNEL_WHITE: or-ed into a kernel id, theta gains log w as its last entry


class GpryAffine(C.Structure):
    _fields_ = [("has_x_affine", C.c_int),
                ("x_lo", C.c_double * GPRY_MAX_DIM),
                ("x_span", C.c_double * GPRY_MAX_DIM),
                ("y_mean", C.c_double), ("y_std", C.c_double),
                ("clip_hi", C.c_double)]


class GpryCand(C.Structure):
    _fields_ = [("acq", C.c_double), ("y", C.c_double), ("sigma", C.c_double),
                ("idx", C.c_int64)]


CAND_DTYPE = np.dtype([("acq", "<f8"), ("y", "<f8"), ("sigma", "<f8"), ("idx", "<i8")])

_P = C.POINTER
_dp = _P(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); mirrors include/gpry_hip.h one to one
SIGNATURES = {
    "gpry_version": (C.c_int, []),
    "gpry_device_count": (C.c_int, [_P(C.c_int)]),
    "gpry_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, _P(C.c_int64), _P(C.c_int),
                                   _P(C.c_int), C.c_char_p, C.c_int]),
    "gpry_ctx_create": (C.c_int, [C.c_int, _P(_vp)]),
    "gpry_ctx_destroy": (C.c_int, [_vp]),
    "gpry_last_error": (C.c_char_p, [_vp]),
    "gpry_ctx_sync": (C.c_int, [_vp]),
    "gpry_ctx_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "gpry_ctx_get_option": (C.c_int, [_vp, C.c_char_p, _vp]),
    "gpry_set_train": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int]),
    "gpry_set_theta": (C.c_int, [_vp, C.c_int, _vp]),
    "gpry_set_affine": (C.c_int, [_vp, _P(GpryAffine)]),
    "gpry_kernel_train": (C.c_int, [_vp, C.c_int, _vp]),
    "gpry_kernel_cross": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "gpry_factorize": (C.c_int, [_vp, _P(C.c_int)]),
    "gpry_get_factor": (C.c_int, [_vp, _vp, _vp, _vp]),
    "gpry_append_rows": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _P(C.c_int)]),
    "gpry_lml": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_double), _vp, _P(C.c_int)]),
    "gpry_lml_batch": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),
    "gpry_loo_objective": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_double), _vp, _P(C.c_int)]),
    "gpry_loo_objective_batch": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),
    "gpry_lml_hessian": (C.c_int, [_vp, _vp, _P(C.c_double), _vp, _vp, _P(C.c_int), _P(C.c_double)]),
    "gpry_predict": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "gpry_debug_serve_stats": (C.c_int, [_vp, _P(C.c_int64), _P(C.c_int64)]),
    "gpry_ns_prior": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_int64, _vp, _vp, _P(C.c_double)]),
    "gpry_ns_generation": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double, _vp, C.c_uint64, C.c_int64,
                                     C.c_int, C.c_int, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_ns_generation_clustered": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double, _vp, C.c_uint64,
                                               C.c_int64, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp,
                                               _P(C.c_double)]),
    "gpry_ns_generation_volumes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double, _vp, C.c_uint64,
                                             C.c_int64, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp,
                                             _P(C.c_double)]),
    "gpry_ns_generation_phantoms": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_double, _vp, C.c_uint64,
                                              C.c_int64, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int,
                                              _vp, _vp, _P(C.c_double)]),
    "gpry_ns_knn": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _P(C.c_double)]),
    "gpry_mcmc_chains": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_double, C.c_double, C.c_uint64,
                                   C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_mcmc_ladders": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp, C.c_double, C.c_uint64,
                                    C.c_int64, C.c_int, C.c_int, C.c_int] + [_vp] * 11 + [_P(C.c_double)]),
    "gpry_hmc_chains": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_double, C.c_int, C.c_double, C.c_double,
                                  C.c_uint64, C.c_int64, C.c_int, C.c_int] + [_vp] * 12),
    "gpry_hmc_chains_reflect": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_double, C.c_int, C.c_double,
                                          C.c_double, C.c_uint64, C.c_int64, C.c_int, C.c_int] + [_vp] * 11
                                + [C.c_int, C.c_int, _vp, _vp]),
    "gpry_maximize_mean": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_double,
                                     C.c_double, C.c_double] + [_vp] * 12 + [_P(C.c_double)]),
    "gpry_maximize_acq": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int,
                                    C.c_int, C.c_double, C.c_double, C.c_double] + [_vp] * 14 + [_P(C.c_double)]),
    "gpry_hessian_mean": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_mean_theta_grad": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _P(C.c_double)]),
    "gpry_predict_thetas": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_predict_thetas_var": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_predict_cov": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_sample_joint": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_uint64, C.c_double, _vp, _vp, _vp, _vp,
                                    _P(C.c_int), _P(C.c_double), _P(C.c_double)]),
    "gpry_loo": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_svm_fit": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int64, _vp,
                               _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_int64), _P(C.c_int), _P(C.c_double)]),
    "gpry_leave_out": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_predict_without": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _P(C.c_double)]),
    "gpry_var_theta_grad": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _P(C.c_double)]),
    "gpry_var_theta_grad_panel": (C.c_int64, [_vp]),
    "gpry_predict_grad": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "gpry_predict_grad_batch": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp, _vp]),
    "gpry_predict_point": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "gpry_set_gates": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_int, _vp]),
    "gpry_sweep_logexp": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_double, C.c_double,
                                    C.c_double, _vp, _vp, _vp, _P(C.c_int64)]),
    "gpry_sweep_logexp_given": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_double, C.c_double,
                                          C.c_double, _vp, _vp, _vp, _P(C.c_int64)]),
    "gpry_sweep_fetch": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp]),
    "gpry_sweep_prune_info": (C.c_int, [_vp, _vp, _vp]),
    "gpry_sweep_screen_info": (C.c_int, [_vp, _vp]),
    "gpry_sweep_topk": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, _P(C.c_int64),
                                  _P(C.c_double)]),
    "gpry_kb_reset": (C.c_int, [_vp]),
    "gpry_kb_register": (C.c_int, [_vp, _vp, C.c_int64, _P(C.c_int64), _vp]),
    "gpry_kb_gram": (C.c_int, [_vp, C.c_int64, _vp, _vp, _P(C.c_int64)]),
    "gpry_kb_gram_rows": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _P(C.c_int64)]),
    "gpry_kb_rank": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp,
                               C.c_int64, _vp, _vp, _vp, _vp, _vp, _P(C.c_int64), _P(C.c_int64), _vp]),
    "gpry_comm_unique_id": (C.c_int, [_vp]),
    "gpry_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _P(_vp)]),
    "gpry_comm_destroy": (C.c_int, [_vp]),
    "gpry_comm_info": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "gpry_comm_allgather": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "gpry_comm_allreduce_max": (C.c_int, [_vp, _vp, C.c_int64]),
    "gpry_comm_barrier": (C.c_int, [_vp]),
    "gpry_group_create": (C.c_int, [C.c_int, _P(C.c_int), _vp, _P(_vp)]),
    "gpry_group_destroy": (C.c_int, [_vp]),
    "gpry_group_size": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "gpry_group_member": (_vp, [_vp, C.c_int]),
    "gpry_group_last_error": (C.c_char_p, [_vp]),
    "gpry_group_set_model": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, C.c_int, _vp,
                                       _P(GpryAffine), _P(C.c_int)]),
    "gpry_group_set_gates": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_int, _vp]),
    "gpry_group_sweep_logexp": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_double, C.c_double,
                                          C.c_double, _vp, _vp, _vp, _P(C.c_int64)]),
    "gpry_group_sweep_logexp_given": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_double, C.c_double,
                                                C.c_double, _vp, _vp, _vp, _P(C.c_int64)]),
    "gpry_group_sweep_fetch": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp]),
    "gpry_group_sweep_topk": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, _P(C.c_int64),
                                        _P(C.c_double), _P(C.c_int)]),
    "gpry_group_lml_batch": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "gpry_timing_reset": (C.c_int, [_vp]),
    "gpry_timing_get": (C.c_int, [_vp, C.c_char_p, _P(C.c_double), _P(C.c_int64)]),
    "gpry_sweep_info": (C.c_int, [_vp, _P(C.c_int), _vp]),
    "gpry_microbench": (C.c_int, [_vp, C.c_int, C.c_int64, _P(C.c_double)]),
    "gpry_debug_gemm": (C.c_int, [_vp, _vp, _vp, _vp] + [C.c_int] * 9),
    "gpry_debug_logexp": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_double, C.c_double, C.c_double, _vp]),
}


def _given_arrays(y_given, sigma_given, M):
    """The sampler's own (y, sigma_y) as contiguous float64 arrays of M rows; sigma without y is not a case of the
    reference (it is recomputed there: the caller passes neither)."""
    if y_given is None:
        raise ValueError("sigma_given without y_given")
    y_given = np.ascontiguousarray(y_given, dtype=np.float64)
    if y_given.shape != (M,):
        raise ValueError(f"y_given has shape {y_given.shape}, the pool has {M} rows")
    if sigma_given is not None:
        sigma_given = np.ascontiguousarray(sigma_given, dtype=np.float64)
        if sigma_given.shape != (M,):
            raise ValueError(f"sigma_given has shape {sigma_given.shape}, the pool has {M} rows")
    return y_given, sigma_given


# status codes of gpry_maximize_mean
MAX_STATUS = ("CONVERGED_G", "CONVERGED_F", "STALLED", "MAXITER", "BAD_START", "BAD_GRADIENT")


class GpryHipError(RuntimeError):
    """An API / HIP / RCCL failure reported by libgpry_hip.so."""


_lib = None


def load_library(path=None):
    """Load (once) and return the shared library.  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("GPRY_HIP_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise GpryHipError(
            f"{p} not found. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C gpry_amd/csrc`. There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptrs(arrays, *keys):
    """The pointers of ``arrays[key]`` in the order of ``keys``, NULL for a key that is not there."""
    return [_ptr(arrays.get(k)) for k in keys]


# the output arguments that the chain entry points / the maximisers have in common, in the order of the C prototypes
_CHAIN_OUT = ("X", "y", "X_last", "y_last", "naccept", "ncalls")
_BFGS_OUT = ("iters", "ncalls", "ngrad", "status")
_BFGS_TR = ("G_tr", "nhalv_tr", "reset_tr")


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def device_count():
    n = C.c_int(0)
    lib = load_library()
    if lib.gpry_device_count(C.byref(n)) != 0:
        return 0
    return n.value


def make_affine(x_lo=None, x_span=None, y_mean=0.0, y_std=1.0, clip_hi=np.inf):
    tf = GpryAffine()
    tf.has_x_affine = 0 if x_lo is None else 1
    if x_lo is not None:
        for k in range(len(x_lo)):
            tf.x_lo[k] = float(x_lo[k])
            tf.x_span[k] = float(x_span[k])
    tf.y_mean, tf.y_std = float(y_mean), float(y_std)
    tf.clip_hi = float(clip_hi)
    return tf


class Device:
    """One ``gpry_ctx``: the device-resident GP state of one GPU.  Like the context it wraps, a ``Device`` is not
    re-entrant: one thread at a time (distinct ``Device`` objects may be driven from distinct threads)."""

    applies_gates_in_predict = True     # option "predict_gates": gpry_predict ORs the gates of set_gates into the mask

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.gpry_ctx_create(int(device), C.byref(self._h))
        if rc != 0:
            msg = self._lib.gpry_last_error(None).decode(errors="replace")
            self._h = None
            raise GpryHipError(f"gpry_ctx_create(device={device}) failed ({rc}): {msg}. "
                               "The HIP path needs a GPU; there is no CPU fallback.")
        self.device = int(device)
        self.N = 0
        self.d = 0

    @classmethod
    def _view(cls, handle, device):
        """Non-owning wrapper of a context that belongs to a ``DeviceGroup``."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = C.c_void_p(handle)
        self._borrowed = True
        self.device, self.N, self.d = int(device), 0, 0
        return self

    # -- plumbing -------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.gpry_last_error(self._h).decode(errors="replace")
            raise GpryHipError(f"{what} failed ({rc}): {msg}")

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = None
            return
        if getattr(self, "_h", None):
            try:
                self._lib.gpry_ctx_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    def __del__(self):
        self.close()

    def sync(self):
        self._check(self._lib.gpry_ctx_sync(self._h), "gpry_ctx_sync")

    def set_option(self, key, value):
        self._check(self._lib.gpry_ctx_set_option(self._h, key.encode(), int(value)),
                    "gpry_ctx_set_option")

    def get_option(self, key):
        v = C.c_int64(0)
        self._check(self._lib.gpry_ctx_get_option(self._h, key.encode(), C.byref(v)), "gpry_ctx_get_option")
        return v.value

    @property
    def lml_batch_max(self):
        """Largest training set whose ``lml_batch`` runs as ONE chain of launches (option ``lml_batch``; up to 128 points
        the single-launch objective serves a batch whatever this says)."""
        return self.get_option("lml_batch")

    def info(self):
        name = C.create_string_buffer(256)
        arch = C.create_string_buffer(256)
        hbm, ncu, clk = C.c_int64(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.gpry_device_info(self.device, name, 256, C.byref(hbm), C.byref(ncu),
                                               C.byref(clk), arch, 256), "gpry_device_info")
        return {"name": name.value.decode(), "arch": arch.value.decode(),
                "hbm_bytes": hbm.value, "n_cu": ncu.value, "clock_khz": clk.value}

    # -- model state ----------------------------------------------------------------
    def set_train(self, X_, y_, alpha):
        X_ = _f64(X_)
        N, d = X_.shape
        y_ = _f64(y_, (N,))
        alpha = _f64(np.broadcast_to(alpha, (N,)))
        self._check(self._lib.gpry_set_train(self._h, _ptr(X_), _ptr(y_), _ptr(alpha), N, d),
                    "gpry_set_train")
        self.N, self.d = N, d

    def set_theta(self, kernel_id, theta):
        """``kernel_id``: 0..3, or-ed with ``KERNEL_WHITE`` for a model with a fitted white term; ``theta`` is then
        ``[log C, log l_1 .. l_d, log w]``, and so is every theta / gradient of ``lml`` and ``lml_batch``."""
        white = bool(int(kernel_id) & KERNEL_WHITE)
        theta = _f64(theta, (self.d + 1 + white,))
        self._check(self._lib.gpry_set_theta(self._h, int(kernel_id), _ptr(theta)),
                    "gpry_set_theta")
        self.white = white

    @property
    def n_theta(self):
        return self.d + 1 + int(getattr(self, "white", False))

    def set_affine(self, x_lo=None, x_span=None, y_mean=0.0, y_std=1.0, clip_hi=np.inf):
        tf = make_affine(x_lo, x_span, y_mean, y_std, clip_hi)
        self._check(self._lib.gpry_set_affine(self._h, C.byref(tf)), "gpry_set_affine")

    # -- kernels --------------------------------------------------------------------
    def kernel_train(self, add_alpha=False):
        K = np.empty((self.N, self.N))
        self._check(self._lib.gpry_kernel_train(self._h, int(bool(add_alpha)), _ptr(K)),
                    "gpry_kernel_train")
        return K

    def kernel_cross(self, Xc_):
        Xc_ = _f64(Xc_)
        M = Xc_.shape[0]
        K = np.empty((M, self.N))
        if M:
            self._check(self._lib.gpry_kernel_cross(self._h, _ptr(Xc_), M, _ptr(K)),
                        "gpry_kernel_cross")
        return K

    # -- factor / lml ---------------------------------------------------------------
    def factorize(self):
        info = C.c_int(0)
        self._check(self._lib.gpry_factorize(self._h, C.byref(info)), "gpry_factorize")
        return info.value

    def append_rows(self, Xnew_, ynew_, alphanew):
        """Extend the factor by the rows ``Xnew_`` (bordered update, fixed theta).  Returns ``info``."""
        Xnew_ = _f64(np.atleast_2d(Xnew_))
        k = Xnew_.shape[0]
        if Xnew_.shape[1] != self.d:
            raise ValueError(f"expected {self.d} columns, got {Xnew_.shape[1]}")
        ynew_ = _f64(ynew_, (k,))
        alphanew = _f64(np.broadcast_to(alphanew, (k,)))
        info = C.c_int(0)
        self._check(self._lib.gpry_append_rows(self._h, _ptr(Xnew_), _ptr(ynew_), _ptr(alphanew), k,
                                               C.byref(info)), "gpry_append_rows")
        if info.value == 0:
            self.N += k
        return info.value

    def get_factor(self, want_L=True, want_V=True, want_alpha=True):
        N = self.N
        L = np.empty((N, N)) if want_L else None
        V = np.empty((N, N)) if want_V else None
        a = np.empty(N) if want_alpha else None
        self._check(self._lib.gpry_get_factor(self._h, _ptr(L), _ptr(V), _ptr(a)),
                    "gpry_get_factor")
        return L, V, a

    def lml(self, theta, eval_gradient=False):
        # persistent argument buffers: at small N an evaluation takes 30-60 us, of which building two arrays and four
        # ctypes pointers per call used to be 3-4
        buf = getattr(self, "_lml_buf", None)
        if buf is None or len(buf[0]) != self.n_theta:
            th, gr = np.zeros(self.n_theta), np.zeros(self.n_theta)
            val, info = C.c_double(0.0), C.c_int(0)
            buf = self._lml_buf = (th, gr, C.c_void_p(th.ctypes.data), C.c_void_p(gr.ctypes.data), val, info,
                                   C.byref(val), C.byref(info))
        th, gr, pth, pgr, val, info, rval, rinfo = buf
        th[:] = theta                          # (raises on a shape mismatch)
        rc = self._lib.gpry_lml(self._h, pth, 1 if eval_gradient else 0, rval, pgr, rinfo)
        if rc != 0:
            self._check(rc, "gpry_lml")
        if eval_gradient:
            return val.value, gr.copy(), info.value
        return val.value, info.value

    def _theta_vec(self, theta):
        theta = _f64(np.asarray(theta, dtype=np.float64).ravel())
        if theta.shape[0] != self.n_theta:
            raise ValueError(f"expected {self.n_theta} entries, got {theta.shape[0]}")
        return theta

    def _theta_rows(self, thetas):
        thetas = _f64(np.atleast_2d(thetas))
        if thetas.shape[1] != self.n_theta:
            raise ValueError(f"expected {self.n_theta} columns, got {thetas.shape[1]}")
        return thetas

    def loo_objective(self, theta, eval_gradient=False):
        """The leave-one-out log predictive density of the training targets at ``theta`` (gpry_loo_objective), transformed
        units like ``lml``: ``(value, info)`` or ``(value, grad, info)``; ``(-inf, zeros, info > 0)`` where the matrix
        is not positive definite.  The factor held for prediction is not disturbed."""
        theta = self._theta_vec(theta)
        grad = np.zeros(self.n_theta)
        val, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gpry_loo_objective(self._h, _ptr(theta), 1 if eval_gradient else 0, C.byref(val), _ptr(grad),
                                                 C.byref(info)), "gpry_loo_objective")
        if eval_gradient:
            return val.value, grad, info.value
        return val.value, info.value

    def lml_hessian(self, theta):
        """Log marginal likelihood, its gradient and its Hessian in theta at ``theta`` (gpry_lml_hessian), transformed
        units: a dict ``lml``, ``grad`` (n_theta,), ``H`` (n_theta, n_theta; symmetric to the last bit), ``info``,
        ``device_ms``.  ``lml`` and ``grad`` have the bits of ``lml(theta, True)``; ``(-inf, zeros, zeros, info > 0)``
        where the matrix is not positive definite.  Models of more than 4096 padded rows are refused.  The factor held
        for prediction is not disturbed."""
        theta = self._theta_vec(theta)
        grad = np.zeros(self.n_theta)
        H = np.zeros((self.n_theta, self.n_theta))
        val, info, ms = C.c_double(0.0), C.c_int(0), C.c_double(0.0)
        self._check(self._lib.gpry_lml_hessian(self._h, _ptr(theta), C.byref(val), _ptr(grad), _ptr(H), C.byref(info),
                                               C.byref(ms)), "gpry_lml_hessian")
        return {"lml": val.value, "grad": grad, "H": H, "info": info.value, "device_ms": ms.value}

    def _objective_batch(self, symbol, thetas, eval_gradient):
        thetas = self._theta_rows(thetas)
        B, w = thetas.shape
        val = np.empty(B)
        grad = np.zeros((B, w)) if eval_gradient else None
        info = np.zeros(B, dtype=np.int32)
        self._check(getattr(self._lib, symbol)(self._h, _ptr(thetas), B, int(bool(eval_gradient)), _ptr(val), _ptr(grad),
                                               _ptr(info)), symbol)
        return (val, grad, info) if eval_gradient else (val, info)

    def loo_objective_batch(self, thetas, eval_gradient=True):
        """``loo_objective`` for every row of ``thetas`` in one call (gpry_loo_objective_batch): ``(value (B,), grad (B,
        n_theta), info (B,))``, or ``(value, info)`` without gradients.  Up to the ``lml_batch`` limit one chain of launches
        carries all rows; every row has the bits of a single ``loo_objective`` call."""
        return self._objective_batch("gpry_loo_objective_batch", thetas, eval_gradient)

    def lml_batch(self, thetas, eval_gradient=True):
        """``lml`` for every row of ``thetas`` in one call: ``(lml (B,), grad (B, 1 + d), info (B,))`` (``(lml, info)``
        without gradients).  N <= 128, d <= 16: one launch, one workgroup per theta, the bits of single ``lml`` calls."""
        return self._objective_batch("gpry_lml_batch", thetas, eval_gradient)

    # -- predict / sweep ------------------------------------------------------------
    def predict(self, X, return_std=False, mask=None):
        if not return_std and mask is None and 0 < len(X) <= 8:
            # the point-by-point callers (nested samplers, MCMC): persistent buffers and cached pointers -- building
            # four ctypes pointers and two arrays per call cost more than the device round trip
            fast = getattr(self, "_small", None)
            if fast is None or fast[0].shape[1] != self.d:
                xin, out = np.zeros((8, max(self.d, 1))), np.zeros(8)
                fast = self._small = (xin, out, C.c_void_p(xin.ctypes.data), C.c_void_p(out.ctypes.data))
            xin, out, pin, pout = fast
            M = len(X)
            if np.ndim(X) != 2 or np.shape(X)[1] != self.d:      # (an assignment would broadcast a vector or a column)
                raise ValueError(f"expected an (M, {self.d}) array, got shape {np.shape(X)}")
            xin[:M] = X            # (converts dtype / strides)
            rc = self._lib.gpry_predict(self._h, pin, M, None, pout, None)
            if rc != 0:
                self._check(rc, "gpry_predict")
            return out[:M].copy()
        X = _f64(X)
        M = X.shape[0]
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected an array of shape (M, {self.d}), got {X.shape}")
        mean = np.empty(M)
        std = np.empty(M) if return_std else None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if M:
            self._check(self._lib.gpry_predict(self._h, _ptr(X), M, _ptr(mask), _ptr(mean),
                                               _ptr(std)), "gpry_predict")
        return (mean, std) if return_std else mean

    def serve_stats(self):
        """(launches, requests) of the resident predict kernel that answers small mean-only ``predict`` calls."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.gpry_debug_serve_stats(self._h, C.byref(a), C.byref(b)), "gpry_debug_serve_stats")
        return a.value, b.value

    # -- nested sampling of the mean (gpry_amd/nested.py drives these two) ----------------
    def ns_prior(self, lo, hi, seed, n):
        """``n`` points uniform on the box [lo, hi] and their ``predict`` values: ``(X (n, d), y (n,), device_ms)``."""
        lo, hi = _f64(lo, (self.d,)), _f64(hi, (self.d,))
        X, y, ms = np.empty((int(n), self.d)), np.empty(int(n)), C.c_double(0.0)
        self._check(self._lib.gpry_ns_prior(self._h, _ptr(lo), _ptr(hi), int(seed), int(n), _ptr(X), _ptr(y),
                                            C.byref(ms)), "gpry_ns_prior")
        return X, y, ms.value

    def _ns_generate(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels, cum_p, thin=None):
        """One generation call: checks the arguments, picks the entry point from (labels, cum_p, thin) -- plain,
        _clustered, _volumes; _phantoms whenever ``thin`` is given -- and returns ``(X_new, y_new, ncalls, X_ph, y_ph,
        device_ms)``, X_ph and y_ph None without ``thin``."""
        if cum_p is not None and labels is None:
            raise ValueError("cum_p needs labels")
        lo, hi = _f64(lo, (self.d,)), _f64(hi, (self.d,))
        X_surv = _f64(X_surv)
        n = X_surv.shape[0]
        if X_surv.ndim != 2 or X_surv.shape[1] != self.d:
            raise ValueError(f"expected survivors of shape (n, {self.d}), got {X_surv.shape}")
        y_surv = _f64(y_surv, (n,))
        k, num_repeats = int(k), int(num_repeats)
        lab = cp = None
        nc = 1
        if labels is None:
            W = _f64(W, (self.d, self.d))
        else:
            W = _f64(W)
            if W.ndim != 3 or W.shape[1:] != (self.d, self.d):
                raise ValueError(f"expected W of shape (n_clusters, {self.d}, {self.d}), got {W.shape}")
            nc = int(W.shape[0])
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.shape != (n,):
                raise ValueError(f"expected {n} labels, got shape {lab.shape}")
            if cum_p is not None:
                cp = _f64(cum_p, (nc,))
        X_new, y_new, cnt, ms = np.empty((k, self.d)), np.empty(k), np.zeros(k, np.int64), C.c_double(0.0)
        X_ph = y_ph = None
        out = [_ptr(X_new), _ptr(y_new), _ptr(cnt)]
        if thin is not None:
            thin = int(thin)
            n_ph = max(num_repeats - 1, 0) // max(thin, 1)          # (thin < 1 is refused by the library)
            X_ph, y_ph = np.empty((k, n_ph, self.d)), np.empty((k, n_ph))
            name, own = "gpry_ns_generation_phantoms", [_ptr(lab), nc, _ptr(cp)]
            out += [thin, _ptr(X_ph), _ptr(y_ph)]
        elif lab is None:
            name, own = "gpry_ns_generation", []
        elif cp is None:
            name, own = "gpry_ns_generation_clustered", [_ptr(lab), nc]
        else:
            name, own = "gpry_ns_generation_volumes", [_ptr(lab), nc, _ptr(cp)]
        # (every entry point: the common arguments, its own, the outputs)
        self._check(getattr(self._lib, name)(self._h, _ptr(lo), _ptr(hi), _ptr(X_surv), _ptr(y_surv), n, float(lstar),
                                             _ptr(W), int(seed), int(generation), k, num_repeats, *own, *out,
                                             C.byref(ms)), name)
        return X_new, y_new, cnt, X_ph, y_ph, ms.value

    def ns_generation(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels=None,
                      cum_p=None):
        """One generation of ``k`` slice-sampling chains above ``lstar``: ``(X_new (k, d), y_new (k,), ncalls (k,),
        device_ms)``.  ``W`` (d, d) is lower triangular (``nested.whitening`` / ``cholesky_ridged`` deliver one): the
        direction is tril(W) z / |z|, entries above the diagonal are not read.  ``labels`` (nsurv cluster numbers) with
        ``W`` of shape (n_clusters, d, d): every chain walks with the matrix of its starting survivor's cluster
        (gpry_ns_generation_clustered).  With ``cum_p`` (n_clusters cumulative probabilities, the last 1.0) as well,
        every chain first draws its cluster from cum_p and then its start among that cluster's survivors
        (gpry_ns_generation_volumes)."""
        out = self._ns_generate(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels, cum_p)
        return out[:3] + out[5:]

    def ns_generation_phantoms(self, lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, thin,
                               labels=None, cum_p=None):
        """``ns_generation`` that also keeps the chains' interior states: ``(X_new (k, d), y_new (k,), ncalls (k,), X_ph
        (k, n_ph, d), y_ph (k, n_ph), device_ms)``, n_ph = (num_repeats - 1) // thin.  Slot i of chain c is its state
        after step (i + 1) thin; the last state is X_new and is not among them.  X_new, y_new and ncalls are those of
        ``ns_generation`` with the same arguments, bit for bit (gpry_ns_generation_phantoms)."""
        return self._ns_generate(lo, hi, X_surv, y_surv, lstar, W, seed, generation, k, num_repeats, labels, cum_p, thin)

    def ns_knn(self, lo, hi, X, k):
        """The ``k`` nearest other points of every row of ``X`` in unit-cube coordinates, in order of (squared distance,
        index): ``(nbr (n, k) int32, device_ms)`` (gpry_ns_knn)."""
        lo, hi = _f64(lo, (self.d,)), _f64(hi, (self.d,))
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (n, {self.d}), got {X.shape}")
        n, k = X.shape[0], int(k)
        nbr, ms = np.empty((n, max(k, 0)), np.int32), C.c_double(0.0)
        self._check(self._lib.gpry_ns_knn(self._h, _ptr(lo), _ptr(hi), _ptr(X), n, k, _ptr(nbr), C.byref(ms)),
                    "gpry_ns_knn")
        return nbr, ms.value

    # -- what the chain and the maximiser wrappers below share ---------------------------------
    def _starts(self, X0, what="start states", count="nchains"):
        """``X0`` as a contiguous (count, d) float64 array."""
        X0 = _f64(X0)
        if X0.ndim != 2 or X0.shape[1] != self.d:
            raise ValueError(f"expected {what} of shape ({count}, {self.d}), got {X0.shape}")
        return X0

    @staticmethod
    def _chain_out(n, d, nsteps, thin, proposals, **own):
        """The output dict of a chain call: the records, the last states and the counters, then the entry point's
        ``own`` arrays, then (``proposals``) ``X_prop`` / ``y_prop``."""
        nrec = nsteps // thin if thin > 0 else 0
        out = dict(X=np.empty((n, nrec, d)), y=np.empty((n, nrec)), X_last=np.empty((n, d)), y_last=np.empty(n),
                   naccept=np.zeros(n, np.int64), ncalls=np.zeros(n, np.int64), **own)
        if proposals:
            out.update(X_prop=np.empty((n, nsteps, d)), y_prop=np.empty((n, nsteps)))
        return out

    def _bfgs_io(self, X0, fixed, H0, max_iter, hooks, values):
        """Checked (X0, fixed, H0) of a maximiser call, its output dict -- ``X``, the ``values`` (nstart,), ``G``, the
        counters and ``status`` -- and the trace dict (empty without ``hooks``; the value's trace is values[0] + "_tr")."""
        X0 = self._starts(X0, "starts", "nstart")
        n, d = X0.shape
        H0 = _f64(H0, (d, d))
        fixed = np.ascontiguousarray(fixed)
        if fixed.shape != (d,) or fixed.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
            raise ValueError(f"expected a boolean mask of shape ({d},), got {fixed.dtype} {fixed.shape}")
        out = dict(X=np.empty((n, d)), **{v: np.empty(n) for v in values}, G=np.empty((n, d)), iters=np.zeros(n, np.int32),
                   ncalls=np.zeros(n, np.int64), ngrad=np.zeros(n, np.int64), status=np.zeros(n, np.int32))
        tr = {}
        if hooks:
            m = max(max_iter, 0)
            tr = {"U_tr": np.empty((n, m + 1, d)), values[0] + "_tr": np.empty((n, m + 1)), "G_tr": np.empty((n, m + 1, d)),
                  "nhalv_tr": np.empty((n, m), np.int32), "reset_tr": np.empty((n, m), np.int32)}
        return X0, fixed.astype(np.uint8), H0, out, tr

    # -- Metropolis MCMC of the mean (gpry_amd/mcmc.py drives this one) ---------------------
    def mcmc_chains(self, lo, hi, X0, y0, Lp, T, minus_inf_value, seed, batch, nsteps, thin, proposals=False):
        """``nsteps`` Metropolis steps of ``len(X0)`` chains from the states (X0, y0) (y0 NaN: evaluated first), proposal
        u' = u + Lp z in unit-cube coordinates: a dict with ``X`` (nchains, nsteps // thin, d) and ``y`` (nchains,
        nsteps // thin), the states after every thin-th step; ``X_last`` / ``y_last``, ``naccept`` / ``ncalls`` per chain;
        ``device_ms``; with ``proposals`` also ``X_prop`` (nchains, nsteps, d) and ``y_prop`` (NaN: not evaluated)."""
        lo, hi, X0 = _f64(lo, (self.d,)), _f64(hi, (self.d,)), self._starts(X0)
        n, d = X0.shape
        y0, Lp = _f64(y0, (n,)), _f64(Lp, (d, d))
        nsteps, thin = int(nsteps), int(thin)
        out = self._chain_out(n, d, nsteps, thin, proposals)
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_mcmc_chains(self._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), n, _ptr(Lp), float(T),
                                               float(minus_inf_value), int(seed), int(batch), nsteps, thin,
                                               *_ptrs(out, *_CHAIN_OUT, "X_prop", "y_prop"), C.byref(ms)),
                    "gpry_mcmc_chains")
        out["device_ms"] = ms.value
        return out

    # -- tempered Metropolis ladders of the mean (gpry_amd/tempering.py drives this one) ------
    def mcmc_ladders(self, lo, hi, X0, y0, nrungs, Lp, T, minus_inf_value, seed, batch, nsteps, thin, swap_every,
                     proposals=False):
        """``nsteps`` Metropolis steps of ``len(X0) // nrungs`` ladders of ``nrungs`` chains (chain a * nrungs + r is slot r
        of ladder a) with the proposal factors Lp (nrungs, d, d) and temperatures T (nrungs,), a swap round between
        adjacent slots after every ``swap_every``-th step (0: none): the dict of ``mcmc_chains`` over all chains plus
        ``nswap_try`` / ``nswap_acc`` (nladders, nrungs - 1); with ``proposals`` also ``X_prop``, ``y_prop`` and
        ``swap_log`` (nladders, nsteps // swap_every, nrungs - 1): 1 accepted, 0 rejected, -1 not tried
        (gpry_mcmc_ladders)."""
        lo, hi, X0 = _f64(lo, (self.d,)), _f64(hi, (self.d,)), self._starts(X0)
        nrungs = int(nrungs)
        n, d = X0.shape
        if nrungs < 1 or n % nrungs:
            raise ValueError(f"{n} start states do not form ladders of nrungs = {nrungs}")
        nl = n // nrungs
        y0, Lp, T = _f64(y0, (n,)), _f64(Lp, (nrungs, d, d)), _f64(T, (nrungs,))
        nsteps, thin, swap_every = int(nsteps), int(thin), int(swap_every)
        out = self._chain_out(n, d, nsteps, thin, proposals, nswap_try=np.zeros((nl, nrungs - 1), np.int64),
                              nswap_acc=np.zeros((nl, nrungs - 1), np.int64))
        log = None
        if proposals:
            out["swap_log"] = np.full((nl, nsteps // swap_every if swap_every > 0 else 0, nrungs - 1), -1, np.int8)
            log = out["swap_log"] if swap_every > 0 else None
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_mcmc_ladders(self._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), nl, nrungs, _ptr(Lp),
                                                _ptr(T), float(minus_inf_value), int(seed), int(batch), nsteps, thin,
                                                swap_every, *_ptrs(out, *_CHAIN_OUT, "nswap_try", "nswap_acc", "X_prop",
                                                                   "y_prop"), _ptr(log), C.byref(ms)), "gpry_mcmc_ladders")
        out["device_ms"] = ms.value
        return out

    # -- Hamiltonian Monte Carlo of the mean (gpry_amd/hmc.py drives this one) ---------------
    def hmc_chains(self, lo, hi, X0, y0, Lp, eps, nleap, T, minus_inf_value, seed, batch, nsteps, thin, hooks=False,
                   reflect=False, max_reflect=64):
        """``nsteps`` leapfrog trajectories (``nleap`` steps of size ``eps``, jittered, mass-matrix inverse Lp Lp^T in
        unit-cube coordinates) of ``len(X0)`` chains from the states (X0, y0) (y0 NaN: evaluated first): the dict of
        ``mcmc_chains`` plus ``ngrad``, the gradient evaluations per chain (``ncalls``: evaluations of the mean); with
        ``hooks`` also ``X_prop`` (nchains, nsteps, d), ``y_prop`` and ``dH_prop`` (nchains, nsteps; NaN: the trajectory
        was cut short and not evaluated) and ``G0`` (nchains, d), the gradient at the start states (gpry_hmc_chains).
        ``reflect``: the drifts reflect at the walls of the box, at most ``max_reflect`` (1 .. 1024) times each, instead of
        rejecting the trajectory that leaves it, and the dict gains ``nreflect``, the reflections per chain
        (gpry_hmc_chains_reflect)."""
        lo, hi, X0 = _f64(lo, (self.d,)), _f64(hi, (self.d,)), self._starts(X0)
        n, d = X0.shape
        y0, Lp = _f64(y0, (n,)), _f64(Lp, (d, d))
        nsteps, thin = int(nsteps), int(thin)
        out = self._chain_out(n, d, nsteps, thin, hooks, ngrad=np.zeros(n, np.int64))
        if hooks:
            out.update(dH_prop=np.empty((n, nsteps)), G0=np.empty((n, d)))
        ms = C.c_double(0.0)
        name, own = "gpry_hmc_chains", []
        if reflect:
            out["nreflect"] = np.zeros(n, np.int64)
            name, own = "gpry_hmc_chains_reflect", [1, int(max_reflect), _ptr(out["nreflect"])]
        self._check(getattr(self._lib, name)(self._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), n, _ptr(Lp), float(eps),
                                             int(nleap), float(T), float(minus_inf_value), int(seed), int(batch), nsteps,
                                             thin, *_ptrs(out, *_CHAIN_OUT, "ngrad", "X_prop", "y_prop", "dH_prop", "G0"),
                                             *own, C.byref(ms)), name)
        out["device_ms"] = ms.value
        return out

    # -- maximisation of the mean (gpry_amd/maximize.py drives this one) -----------------------
    def maximize_mean(self, lo, hi, X0, y0, fixed, H0, max_iter, max_halvings, gtol, ftol, minus_inf_value, hooks=False):
        """Projected BFGS ascents of the mean inside the box from the ``len(X0)`` starts (X0, y0) (y0 NaN: evaluated
        first); ``fixed`` (d,): the coordinates that keep X0's values; ``H0`` (d, d): the first inverse-Hessian guess and
        reset value, unit-cube coordinates (gpry_maximize_mean).  A dict with ``X`` (nstart, d), ``y``, ``G`` (the
        unit-cube gradient at X), ``iters``, ``ncalls``, ``ngrad``, ``status`` (``MAX_STATUS``) and ``device_ms``; with
        ``hooks`` also the traces ``U_tr`` (nstart, max_iter + 1, d), ``y_tr``, ``G_tr``, ``nhalv_tr`` and ``reset_tr``
        (nstart, max_iter), unused slots NaN / -1."""
        lo, hi = _f64(lo, (self.d,)), _f64(hi, (self.d,))
        max_iter, max_halvings = int(max_iter), int(max_halvings)
        X0, fixed, H0, out, tr = self._bfgs_io(X0, fixed, H0, max_iter, hooks, ("y",))
        n = len(X0)
        y0, ms = _f64(y0, (n,)), C.c_double(0.0)
        self._check(self._lib.gpry_maximize_mean(self._h, _ptr(lo), _ptr(hi), _ptr(X0), _ptr(y0), n, _ptr(fixed), _ptr(H0),
                                                 max_iter, max_halvings, float(gtol), float(ftol), float(minus_inf_value),
                                                 *_ptrs(out, "X", "y", "G", *_BFGS_OUT),
                                                 *_ptrs(tr, "U_tr", "y_tr", *_BFGS_TR), C.byref(ms)), "gpry_maximize_mean")
        out.update(tr)
        out["device_ms"] = ms.value
        return out

    # -- maximisation of the LogExp acquisition (gpry_amd/maximize.py: maximize_acq drives this one) ----
    def maximize_acq(self, lo, hi, X0, fixed, H0, zeta, baseline, sigma_n, max_iter, max_halvings, gtol, ftol,
                     minus_inf_value, hooks=False):
        """Projected BFGS ascents of the LogExp acquisition a = 2 zeta (y - baseline) + log sqrt(sigma^2 - sigma_n^2)
        inside the box from the rows of ``X0``, value and exact gradient evaluated inside the kernel
        (gpry_maximize_acq); ``fixed`` and ``H0`` as in ``maximize_mean``.  A dict with ``X`` (nstart, d), ``a``, ``y``,
        ``sigma`` (at X), ``G`` (the unit-cube gradient of a at X), ``iters``, ``ncalls``, ``ngrad``, ``status``
        (``MAX_STATUS``) and ``device_ms``; with ``hooks`` also the traces ``U_tr`` (nstart, max_iter + 1, d), ``a_tr``,
        ``G_tr``, ``nhalv_tr`` and ``reset_tr`` (nstart, max_iter), unused slots NaN / -1."""
        lo, hi = _f64(lo, (self.d,)), _f64(hi, (self.d,))
        max_iter, max_halvings = int(max_iter), int(max_halvings)
        X0, fixed, H0, out, tr = self._bfgs_io(X0, fixed, H0, max_iter, hooks, ("a", "y", "sigma"))
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_maximize_acq(self._h, _ptr(lo), _ptr(hi), _ptr(X0), len(X0), _ptr(fixed), _ptr(H0),
                                                float(zeta), float(baseline), float(sigma_n), max_iter, max_halvings,
                                                float(gtol), float(ftol), float(minus_inf_value),
                                                *_ptrs(out, "X", "a", "y", "sigma", "G", *_BFGS_OUT),
                                                *_ptrs(tr, "U_tr", "a_tr", *_BFGS_TR), C.byref(ms)), "gpry_maximize_acq")
        out.update(tr)
        out["device_ms"] = ms.value
        return out

    # -- value, gradient and Hessian of the mean (gpry_amd/maximize.py: hessian_gp, laplace_gp drive this one) ----
    def hessian_mean(self, X):
        """Value, gradient and Hessian of the posterior mean at the rows of ``X`` (npts, d), raw coordinates and units of
        y (gpry_hessian_mean): a dict with ``y`` (npts,; ``predict(x[None])`` bit for bit, a gated point is -inf), ``g``
        (npts, d) and ``H`` (npts, d, d), both of the unclipped, ungated mean, H symmetric to the last bit, and
        ``device_ms``.  A Matern-1/2 model is refused."""
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        n, d = X.shape
        out = dict(y=np.empty(n), g=np.empty((n, d)), H=np.empty((n, d, d)))
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_hessian_mean(self._h, _ptr(X), n, _ptr(out["y"]), _ptr(out["g"]), _ptr(out["H"]),
                                                C.byref(ms)), "gpry_hessian_mean")
        out["device_ms"] = ms.value
        return out

    # -- the derivative of the mean in theta (gpry_amd/gpr.py: mean_theta_grad; gpry_amd/hyper.py: hyper_spread) ----
    def mean_theta_grad(self, X):
        """The posterior mean and its derivative in theta = [log C, log l_1 .. log l_d (, log w)] at the rows of ``X``
        (npts, d), raw coordinates (gpry_mean_theta_grad): a dict with ``y`` (npts,; ``predict(x[None])`` bit for bit, a
        gated point is -inf), ``G`` (npts, p; of the unclipped, ungated mean, units of y per unit of log theta) and
        ``device_ms``.  Any number of points; all four kernels."""
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        n = X.shape[0]
        out = dict(y=np.empty(n), G=np.empty((n, self.n_theta)))
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_mean_theta_grad(self._h, _ptr(X), n, _ptr(out["y"]), _ptr(out["G"]), C.byref(ms)),
                    "gpry_mean_theta_grad")
        out["device_ms"] = ms.value
        return out

    # -- the derivative of the variance in theta (gpry_amd/gpr.py: var_theta_grad; gpry_amd/hyper.py: hyper_acq_spread) ----
    def var_theta_grad_panel(self):
        """Points per panel of ``var_theta_grad`` for the model the context holds (gpry_var_theta_grad_panel: a function
        of its padded size alone)."""
        return int(self._lib.gpry_var_theta_grad_panel(self._h))

    def var_theta_grad(self, X, want_var=True):
        """The latent predictive variance and its derivative in theta = [log C, log l_1 .. log l_d (, log w)] at the rows
        of ``X`` (npts, d), raw coordinates (gpry_var_theta_grad): a dict with ``var`` (npts,; y_std^2 (C + w - |V k|^2), not
        clamped, clipped or gated; None with ``want_var=False``), ``G`` (npts, p; units of y^2 per unit of log theta) and
        ``device_ms``.  Any number of points (panels of ``self.var_theta_grad_panel()``); all four kernels; models of at most
        4096 padded rows."""
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        n = X.shape[0]
        out = dict(var=np.empty(n) if want_var else None, G=np.empty((n, self.n_theta)))
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_var_theta_grad(self._h, _ptr(X), n, _ptr(out["var"]), _ptr(out["G"]), C.byref(ms)),
                    "gpry_var_theta_grad")
        out["device_ms"] = ms.value
        return out

    # -- the mean under a batch of thetas (gpry_amd/gpr.py: predict_thetas; gpry_amd/hyper.py: hyper_spread(exact=True)) ----
    def predict_thetas(self, thetas, X, want_var=False):
        """The unclipped, ungated posterior mean at the rows of ``X`` (M, d), raw coordinates, under every row of
        ``thetas`` (B, n_theta; the device's vector) in one call (gpry_predict_thetas): a dict with ``mean`` (B, M),
        ``lml`` (B,; the bits of ``lml(theta, False)``), ``info`` (B,) and ``device_ms``.  A theta whose matrix is not
        positive definite has ``info > 0``, ``lml = -inf`` and a row of NaN.  The model the context holds is not
        disturbed.  Any number of thetas and points; all four kernels.  ``want_var=True`` (gpry_predict_thetas_var): the
        dict has ``var`` (B, M) as well, the predictive variance ``y_std^2 (C_b + w_b - |V_b k_b(x)|^2)`` in untransformed
        units, not clamped at 0; ``mean``, ``lml`` and ``info`` keep their bits."""
        thetas = self._theta_rows(thetas)
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        B, M = thetas.shape[0], X.shape[0]
        out = dict(mean=np.empty((B, M)), lml=np.empty(B), info=np.zeros(B, dtype=np.int32))
        ms = C.c_double(0.0)
        if want_var:
            out["var"] = np.empty((B, M))
            self._check(self._lib.gpry_predict_thetas_var(self._h, _ptr(thetas), B, _ptr(X), M, _ptr(out["mean"]), _ptr(out["var"]),
                                                          _ptr(out["lml"]), _ptr(out["info"]), C.byref(ms)), "gpry_predict_thetas_var")
        else:
            self._check(self._lib.gpry_predict_thetas(self._h, _ptr(thetas), B, _ptr(X), M, _ptr(out["mean"]), _ptr(out["lml"]),
                                                      _ptr(out["info"]), C.byref(ms)), "gpry_predict_thetas")
        out["device_ms"] = ms.value
        return out

    # -- joint posterior covariance and joint draws (gpry_amd/gpr.py: predict(return_cov=True), sample_y; mc.py) ----
    def _joint_args(self, X, mask):
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (m, {self.d}), got {X.shape}")
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (X.shape[0],):
                raise ValueError(f"expected a mask of shape ({X.shape[0]},), got {mask.shape}")
        return X, mask

    def predict_cov(self, X, mask=None):
        """Finalised mean and joint posterior covariance at the rows of ``X`` (m <= 4096, raw coordinates; units of y and
        y^2; gpry_predict_cov): a dict with ``mean`` (m,), ``cov`` (m, m; symmetric to the last bit, the diagonal not
        clamped, zero rows and columns for classifier-rejected points) and ``device_ms``."""
        X, mask = self._joint_args(X, mask)
        m = X.shape[0]
        out = dict(mean=np.empty(m), cov=np.empty((m, m)))
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_predict_cov(self._h, _ptr(X), m, _ptr(mask), _ptr(out["mean"]), _ptr(out["cov"]),
                                               C.byref(ms)), "gpry_predict_cov")
        out["device_ms"] = ms.value
        return out

    def sample_joint(self, X, S, seed, jitter=None, mask=None, want_Z=False, want_Lc=False):
        """``S`` joint draws of the surrogate at the rows of ``X`` (gpry_sample_joint): a dict with ``mean`` (m,; the
        finalised mean), ``Y`` (S, m; centred on the unclipped, ungated mean, -inf in classifier-rejected columns), ``Z``
        and ``Lc`` (the variates and the Cholesky factor, or None), ``jitter_used`` and ``device_ms``.  ``jitter``: the
        first rung of the ladder in units of C y_std^2 (None: 1e-10)."""
        X, mask = self._joint_args(X, mask)
        m, S = X.shape[0], int(S)
        ok = 1 <= S <= 65536 and m >= 1           # (the library refuses; no arrays are made for a request it will refuse)
        out = dict(mean=np.empty(m), Y=np.empty((S, m) if ok else (0, m)),
                   Z=np.empty((S, m)) if want_Z and ok else None, Lc=np.empty((m, m)) if want_Lc and ok else None)
        ms, eps, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gpry_sample_joint(self._h, _ptr(X), m, _ptr(mask), S, int(seed) & (2 ** 64 - 1),
                                                -1.0 if jitter is None else float(jitter), _ptr(out["mean"]),
                                                _ptr(out["Y"]), _ptr(out["Z"]), _ptr(out["Lc"]), C.byref(info),
                                                C.byref(eps), C.byref(ms)), "gpry_sample_joint")
        out["jitter_used"], out["device_ms"] = eps.value, ms.value
        return out

    # -- cross-validation of the training set (gpry_amd/gpr.py: loo, leave_out; mc.py: validate_gp) ------------------
    LOO_OUTPUTS = ("mean", "var_y", "var_f", "seq_mean", "seq_var_y")

    def loo(self, want=LOO_OUTPUTS):
        """Leave-one-out and one-step-ahead predictives of the training targets from the resident factor (gpry_loo), in
        units of y: a dict with ``mean``, ``var_y`` (the predictive of the observation y_i from all other points),
        ``var_f`` (the latent variance, var_y less the point's noise, not below 0), ``seq_mean``, ``seq_var_y`` (y_k from
        the points before it), each (N,) or None where ``want`` leaves it out, and ``device_ms``."""
        out = {k: (np.empty(self.N) if k in want else None) for k in self.LOO_OUTPUTS}
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_loo(self._h, *[_ptr(out[k]) for k in self.LOO_OUTPUTS], C.byref(ms)), "gpry_loo")
        out["device_ms"] = ms.value
        return out

    # -- training of the infinities classifier (gpry_amd/svm.py: SVM(trainer="device")) -------------------------------
    def svm_fit(self, X, finite, C, gamma, eps=1e-3, max_iter=None):
        """The C-SVC dual of the two classes ``finite`` / not, RBF kernel ``exp(-gamma |a - b|^2)``, solved on the device
        (gpry_svm_fit: libsvm's SMO without shrinking).  X: (N, d) in the coordinates the classifier is evaluated in.
        Returns ``alpha`` (N,), ``rho`` (decision(x) = sum_t y_t alpha_t k(x_t, x) - rho with y = +1 for finite),
        ``objective``, ``violation`` (G_max - G_min of the last stop test), ``n_iter``, ``status`` (0 converged, 1 the
        budget of ``max_iter`` updates -- default 100 N + 10000 -- ran out; alpha is feasible either way) and
        ``device_ms``.  The model, sweep, gates and sessions of the context are not touched."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("svm_fit: X must be (N, d)")
        N, d = X.shape
        finite = np.ascontiguousarray(np.asarray(finite).astype(bool), dtype=np.uint8)
        if finite.shape != (N,):
            raise ValueError("svm_fit: finite must be (N,)")
        max_iter = 100 * N + 10000 if max_iter is None else int(max_iter)
        alpha = np.empty(N)
        rho, obj, viol, ms = _ct.c_double(0.0), _ct.c_double(0.0), _ct.c_double(0.0), _ct.c_double(0.0)
        nit, status = _ct.c_int64(0), _ct.c_int(0)
        self._check(self._lib.gpry_svm_fit(self._h, _ptr(X), _ptr(finite), N, d, float(C), float(gamma), float(eps), max_iter,
                                           _ptr(alpha), _ct.byref(rho), _ct.byref(obj), _ct.byref(viol), _ct.byref(nit),
                                           _ct.byref(status), _ct.byref(ms)), "gpry_svm_fit")
        return dict(alpha=alpha, rho=rho.value, objective=obj.value, violation=viol.value, n_iter=int(nit.value),
                    status=int(status.value), device_ms=ms.value)

    @staticmethod
    def _group_arrays(groups):
        """A list of index sequences as gpry_leave_out and gpry_predict_without take it: ``(ngroups, sizes, offsets, idx,
        ok)``; ``ok`` False: the library will refuse the list (none, an empty group or one above 64 indices)."""
        groups = [np.ascontiguousarray(g, dtype=np.int64).reshape(-1) for g in groups]
        ng = len(groups)
        sizes = np.array([len(g) for g in groups], dtype=np.int64)
        offsets = np.zeros(ng + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        idx = np.concatenate(groups) if ng else np.zeros(0, dtype=np.int64)
        ok = ng >= 1 and sizes.min() >= 1 and sizes.max() <= 64     # (the library refuses; no arrays for a refused request)
        return ng, sizes, offsets, idx, bool(ok)

    def predict_without(self, groups, X, want=("dmean", "dvar")):
        """What the model would predict at the rows of ``X`` (M, d; raw coordinates) without each group of training points
        (gpry_predict_without), as a change against the model it holds: a dict with ``dmean`` and ``dvar`` (ngroups, M;
        the change of the unclipped, ungated mean and of the latent variance, units of y and y^2, ``dvar >= 0``; None
        where ``want`` leaves one out), ``info`` (ngroups,; non-zero: the group's block of K^-1 is not positive definite
        and its rows are NaN) and ``device_ms``.  ``groups`` as for ``leave_out``.  Same theta, y map and noise: nothing is
        refactorised, and the model is not disturbed."""
        ng, sizes, offsets, idx, ok = self._group_arrays(groups)
        X = _f64(X)
        if X.ndim != 2 or X.shape[1] != self.d:
            raise ValueError(f"expected points of shape (npts, {self.d}), got {X.shape}")
        if not any(k in want for k in ("dmean", "dvar")):
            raise ValueError("predict_without: want must name dmean or dvar")
        M = X.shape[0]
        shape = (ng, M) if ok and M >= 1 else (0, M)
        out = {k: (np.empty(shape) if k in want else None) for k in ("dmean", "dvar")}
        out["info"] = np.zeros(ng, dtype=np.int32)
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_predict_without(self._h, _ptr(idx), _ptr(offsets), ng, _ptr(X), M, _ptr(out["dmean"]),
                                                   _ptr(out["dvar"]), _ptr(out["info"]), C.byref(ms)), "gpry_predict_without")
        out["device_ms"] = ms.value
        return out

    def leave_out(self, groups):
        """Joint predictive of every group of training targets from the points outside it (gpry_leave_out).  ``groups``: a
        sequence of index sequences (1 to 64 distinct indices each; groups may overlap).  A dict with ``mean`` and ``cov``
        (lists, one (n_g,) and one (n_g, n_g) array per group, in the order of the group's indices, units of y), ``chi2``,
        ``logpdf`` and ``info`` (one per group; info != 0: the group's block of K^-1 was not positive definite and its
        outputs are NaN), ``dof`` and ``device_ms``."""
        ng, sizes, offsets, idx, ok = self._group_arrays(groups)
        mean, cov = np.empty(len(idx) if ok else 0), np.empty(int(np.sum(sizes ** 2)) if ok else 0)
        chi2, logpdf, info = np.empty(ng), np.empty(ng), np.zeros(ng, dtype=np.int32)
        ms = C.c_double(0.0)
        self._check(self._lib.gpry_leave_out(self._h, _ptr(idx), _ptr(offsets), ng, _ptr(mean), _ptr(cov), _ptr(chi2),
                                             _ptr(logpdf), _ptr(info), C.byref(ms)), "gpry_leave_out")
        coff = np.concatenate([[0], np.cumsum(sizes ** 2)])
        return dict(mean=[mean[offsets[g]:offsets[g + 1]] for g in range(ng)],
                    cov=[cov[coff[g]:coff[g + 1]].reshape(sizes[g], sizes[g]) for g in range(ng)],
                    chi2=chi2, logpdf=logpdf, info=info, dof=sizes, device_ms=ms.value)

    def set_gates(self, sv=None, coef=None, gamma=0.0, intercept=0.0, positive_is_finite=True,
                  trust_bounds=None):
        """SVM / trust-region verdicts computed by the device inside ``sweep_logexp``."""
        n_sv = 0
        if sv is not None and len(sv):
            sv = _f64(sv)
            n_sv = sv.shape[0]
            coef = _f64(coef, (n_sv,))
        else:
            sv = coef = None
        tb = None if trust_bounds is None else _f64(trust_bounds, (self.d, 2))
        self._check(self._lib.gpry_set_gates(self._h, _ptr(sv), _ptr(coef), n_sv, float(gamma),
                                             float(intercept), int(bool(positive_is_finite)), _ptr(tb)),
                    "gpry_set_gates")

    def predict_grad(self, x, want_kinv=True, want_kgrad=False, want_mean=True):
        """x-gradient contractions for one point: ``(G^T alpha_, G^T K^-1 k*[, G])``."""
        x = _f64(x, (self.d,))
        mg = np.empty(self.d) if want_mean else None
        kg = np.empty(self.d)
        G = np.empty((self.N, self.d)) if want_kgrad else None
        self._check(self._lib.gpry_predict_grad(self._h, _ptr(x), int(bool(want_kinv)), _ptr(G),
                                                _ptr(mg), _ptr(kg)), "gpry_predict_grad")
        return (mg, kg, G) if want_kgrad else (mg, kg)

    def predict_point(self, x, mask_bits=0, want_kinv=True):
        """``(mean, std, G^T alpha_, G^T K^-1 k*, verdict)`` of ONE point in one call (mean / std finalised as by ``predict``;
        ``verdict``: the mask bits that were applied -- ``mask_bits`` and, with option "predict_gates", the device's own gates).
        Called once per step of an acquisition optimiser: argument buffers and their pointers are kept."""
        buf = getattr(self, "_point_buf", None)
        if buf is None or len(buf[0]) != self.d:
            xin, mg, kg = np.zeros(self.d), np.zeros(self.d), np.zeros(self.d)
            mean, std, bits = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
            buf = self._point_buf = (xin, mg, kg, mean, std, bits, C.c_void_p(xin.ctypes.data), C.byref(mean), C.byref(std),
                                     C.c_void_p(mg.ctypes.data), C.c_void_p(kg.ctypes.data), C.byref(bits))
        xin, mg, kg, mean, std, bits, px, pmean, pstd, pmg, pkg, pbits = buf
        xin[:] = x                                 # (raises on a shape mismatch; converts dtype / strides)
        rc = self._lib.gpry_predict_point(self._h, px, int(mask_bits), 1 if want_kinv else 0, pmean, pstd, pmg, pkg, pbits)
        if rc != 0:
            self._check(rc, "gpry_predict_point")
        return mean.value, std.value, mg.copy(), kg.copy(), bits.value

    def predict_grad_batch(self, X, want_kinv=True):
        """``(mean, std, G^T alpha_, G^T K^-1 k*)`` for every row of ``X`` in one call."""
        X = _f64(np.atleast_2d(X))
        m = X.shape[0]
        mean, std = np.empty(m), np.empty(m)
        mg = np.empty((m, self.d))
        kg = np.zeros((m, self.d))
        if m:
            self._check(self._lib.gpry_predict_grad_batch(self._h, _ptr(X), m, int(bool(want_kinv)), _ptr(mean),
                                                          _ptr(std), _ptr(mg), _ptr(kg)), "gpry_predict_grad_batch")
        return mean, std, mg, kg

    def sweep_logexp(self, X, zeta, baseline, sigma_n, mask=None, M=None, want=("y", "sigma", "acq"),
                     y_given=None, sigma_given=None):
        """Run the fused sweep.  ``X=None`` re-uses the candidate set resident on the device.  ``y_given`` (and
        ``sigma_given``): the sampler's own arrays (``gpry_sweep_logexp_given``) -- y is kept as given and only sigma is
        computed, or with both nothing but the acquisition."""
        if X is not None:
            X = _f64(X)
            M = X.shape[0]
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        out = {k: (np.empty(M) if k in want else None) for k in ("y", "sigma", "acq")}
        n_nan = C.c_int64(0)
        if y_given is None and sigma_given is None:
            self._check(self._lib.gpry_sweep_logexp(
                self._h, _ptr(X), M, _ptr(mask), float(zeta), float(baseline), float(sigma_n),
                _ptr(out["y"]), _ptr(out["sigma"]), _ptr(out["acq"]), C.byref(n_nan)),
                "gpry_sweep_logexp")
        else:
            y_given, sigma_given = _given_arrays(y_given, sigma_given, M)
            self._check(self._lib.gpry_sweep_logexp_given(
                self._h, _ptr(X), M, _ptr(mask), _ptr(y_given), _ptr(sigma_given), float(zeta), float(baseline),
                float(sigma_n), _ptr(out["y"]), _ptr(out["sigma"]), _ptr(out["acq"]), C.byref(n_nan)),
                "gpry_sweep_logexp_given")
        out["n_nan"] = n_nan.value
        self.sweep_epoch = getattr(self, "sweep_epoch", 0) + 1    # the resident arrays changed
        self._sweep_M = M
        return out

    PANEL_FORMS = {0: "none", 1: "mfma", 2: "difference", 3: "small", 4: "hybrid"}

    def sweep_info(self):
        """How the cross-kernel panel of the last sweep / panel predict was built (``gpry_sweep_info``) and the error
        estimates of the model that decided it."""
        form = C.c_int(0)
        est = np.zeros(4)
        self._check(self._lib.gpry_sweep_info(self._h, C.byref(form), _ptr(est)), "gpry_sweep_info")
        return {"panel_form": self.PANEL_FORMS.get(form.value, str(form.value)), "panel_error_estimate": float(est[0]),
                "panel_error_mean_worst_case": float(est[1]), "panel_error_variance": float(est[2]), "panel_gate": float(est[3])}

    def sweep_fetch(self, want=("y", "sigma")):
        """Arrays of the last sweep that are still resident on the device."""
        M = self._sweep_M
        out = {k: (np.empty(M) if k in want else None) for k in ("y", "sigma", "acq")}
        self._check(self._lib.gpry_sweep_fetch(self._h, M, _ptr(out["y"]), _ptr(out["sigma"]),
                                               _ptr(out["acq"])), "gpry_sweep_fetch")
        return out

    PRUNE_INFO = ("pruned", "M", "K_prime", "rounds", "contracted", "completed", "K", "survivors", "y_bound", "live_blocks",
                  "blocks")

    def sweep_prune_info(self):
        """Statistics of the last pruned sweep (option ``sweep_prune``, ``gpry_sweep_prune_info``)."""
        info = np.zeros(len(self.PRUNE_INFO), dtype=np.int64)
        dinfo = np.zeros(5)
        self._check(self._lib.gpry_sweep_prune_info(self._h, _ptr(info), _ptr(dinfo)), "gpry_sweep_prune_info")
        out = {k: int(v) for k, v in zip(self.PRUNE_INFO, info)}
        out["tau"] = float(dinfo[0])
        out["stage_ms"] = dict(zip(("sweep_mean", "sweep_prune_select", "sweep_compact", "sweep_prune_gemm"), dinfo[1:].tolist()))
        return out

    def sweep_screen_info(self):
        """The FP32 screen of the bound pass in the last pruned sweep (option ``sweep_screen``, ``gpry_sweep_screen_info``):
        blocks it certified, and blocks the pass saw."""
        out = np.zeros(2, dtype=np.int64)
        self._check(self._lib.gpry_sweep_screen_info(self._h, _ptr(out)), "gpry_sweep_screen_info")
        return {"certified": int(out[0]), "blocks": int(out[1])}

    def sweep_topk(self, Kp, exclude=None):
        Kp = int(Kp)
        top = np.zeros(max(Kp, 1), dtype=CAND_DTYPE)
        n_out, bound = C.c_int64(0), C.c_double(0.0)
        if exclude is not None and len(exclude):
            exclude = np.ascontiguousarray(np.sort(np.asarray(exclude, dtype=np.int64)))
            nex = len(exclude)
        else:
            exclude, nex = None, 0
        self._check(self._lib.gpry_sweep_topk(self._h, Kp, _ptr(exclude), nex, _ptr(top),
                                              C.byref(n_out), C.byref(bound)), "gpry_sweep_topk")
        return top[:n_out.value], bound.value

    # -- Kriging believer -----------------------------------------------------------
    def kb_reset(self):
        self._check(self._lib.gpry_kb_reset(self._h), "gpry_kb_reset")

    def kb_register(self, X, want_var0=True):
        X = _f64(X)
        m = X.shape[0]
        first = C.c_int64(0)
        var0 = np.empty(m) if want_var0 else None
        self._check(self._lib.gpry_kb_register(self._h, _ptr(X), m, C.byref(first), _ptr(var0)),
                    "gpry_kb_register")
        return first.value, var0

    def kb_gram(self, p, n):
        G, kv = np.empty(n), np.empty(n)
        nn = C.c_int64(0)
        self._check(self._lib.gpry_kb_gram(self._h, int(p), _ptr(G), _ptr(kv), C.byref(nn)),
                    "gpry_kb_gram")
        if nn.value != n:
            raise GpryHipError(f"kb_gram: device holds {nn.value} candidates, host expected {n}")
        return G, kv

    def kb_gram_rows(self, p, n):
        """Gram rows of the registered candidates ``p`` from one launch: ``(G, kv)``, one row per entry of ``p``."""
        p = np.ascontiguousarray(p, dtype=np.int64)
        G, kv = np.empty((len(p), n)), np.empty((len(p), n))
        nn = C.c_int64(0)
        self._check(self._lib.gpry_kb_gram_rows(self._h, _ptr(p), len(p), _ptr(G), _ptr(kv), C.byref(nn)),
                    "gpry_kb_gram_rows")
        if nn.value != n:
            raise GpryHipError(f"kb_gram_rows: device holds {nn.value} candidates, host expected {n}")
        return G, kv

    def kb_rank(self, X_new, var0, idx, y, sigma, acq, order, params, slots):
        """``gpry_kb_rank``: registers ``X_new`` (their ``var0`` is written behind the session's), then ranks the offer into
        the pool ``slots = (idx, y, sigma, acq, acq_cond)`` (int64 / float64 arrays of n_points + 1, updated in place).
        Returns ``(cache_models, info, stats)``: models built, 0 or t + 1 of a non-positive-definite border, and
        (launches, rows, extra requests)."""
        m_new = 0 if X_new is None else len(X_new)
        X_new = None if m_new == 0 else _f64(X_new)
        params = _f64(params)
        counter, info = C.c_int64(0), C.c_int64(0)
        stats = np.zeros(3, dtype=np.int64)
        s_idx, s_y, s_sigma, s_acq, s_cond = slots
        for a, t in ((var0, np.float64), (idx, np.int64), (y, np.float64), (sigma, np.float64), (acq, np.float64),
                     (order, np.int64), (s_idx, np.int64), (s_y, np.float64), (s_sigma, np.float64),
                     (s_acq, np.float64), (s_cond, np.float64)):
            if a.dtype != t or not a.flags.c_contiguous:
                raise ValueError("kb_rank: arrays must be contiguous int64 / float64")
        if not (len(y) == len(sigma) == len(acq) == len(idx)) or len(params) != 5 or \
                not (len(s_idx) == len(s_y) == len(s_sigma) == len(s_acq) == len(s_cond)):
            raise ValueError("kb_rank: array lengths do not match")
        self._check(self._lib.gpry_kb_rank(self._h, _ptr(X_new), m_new, _ptr(var0), len(var0), _ptr(idx), _ptr(y),
                                           _ptr(sigma), _ptr(acq), len(idx), _ptr(order), len(order), _ptr(params),
                                           len(s_idx) - 1, _ptr(s_idx), _ptr(s_y), _ptr(s_sigma), _ptr(s_acq),
                                           _ptr(s_cond), C.byref(counter), C.byref(info), _ptr(stats)), "gpry_kb_rank")
        return counter.value, info.value, stats

    # -- measurement ----------------------------------------------------------------
    def timing_reset(self):
        self._check(self._lib.gpry_timing_reset(self._h), "gpry_timing_reset")

    def timing(self, name):
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        self._lib.gpry_timing_get(self._h, name.encode(), C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value

    def debug_gemm(self, A, B, C0, M, N, K, a_trans=False, b_trans=False, epi=0, kmode=0,
                   lower_only=False, tile_map=0):
        """Unit-test hook for the MFMA GEMM engine (see include/gpry_hip.h)."""
        A, B = _f64(A), _f64(B)
        crow = (M + 127) // 128 if epi == 3 else M
        Cout = np.ascontiguousarray(np.zeros((crow, N)) if C0 is None else C0, dtype=np.float64).copy()
        self._check(self._lib.gpry_debug_gemm(self._h, _ptr(A), _ptr(B), _ptr(Cout), M, N, K,
                                              int(a_trans), int(b_trans), int(epi), int(kmode),
                                              int(lower_only), int(tile_map)), "gpry_debug_gemm")
        return Cout

    def debug_logexp(self, mu, sigma, zeta, baseline, sigma_n):
        """The sweep's acquisition epilogue on given (mean, std) pairs (test hook)."""
        mu, sigma = _f64(mu), _f64(sigma)
        acq = np.empty(len(mu))
        self._check(self._lib.gpry_debug_logexp(self._h, _ptr(mu), _ptr(sigma), len(mu), float(zeta),
                                                float(baseline), float(sigma_n), _ptr(acq)), "gpry_debug_logexp")
        return acq


    def microbench(self, kind, nbytes=0):
        v = C.c_double(0.0)
        self._check(self._lib.gpry_microbench(self._h, int(kind), int(nbytes), C.byref(v)),
                    "gpry_microbench")
        return v.value


class DeviceGroup:
    """Several contexts behind one call (``gpry_group_*``): the sharded sweep of ONE process.

    ``devices``: device indices, repeats allowed (several contexts on one GPU).  ``adopt``: a
    ``Device`` on ``devices[0]`` that becomes member 0 and keeps belonging to its owner (the
    regressor's own context: its factor is used as it is, the other members get the model through
    ``set_model``).  The methods mirror ``Device``'s sweep calls on the whole pool."""

    def __init__(self, devices, adopt=None):
        self._lib = load_library()
        devices = [int(v) for v in devices]
        if not devices:
            raise ValueError("DeviceGroup needs at least one device")
        self.devices = devices
        self._adopt = adopt             # keeps the adopted context alive as long as the group
        arr = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        rc = self._lib.gpry_group_create(len(devices), arr, adopt._h if adopt is not None else None,
                                         C.byref(self._h))
        if rc != 0:
            msg = self._lib.gpry_group_last_error(None).decode(errors="replace")
            self._h = None
            raise GpryHipError(f"gpry_group_create({devices}) failed ({rc}): {msg}")
        n, tr = C.c_int(0), C.c_int(0)
        self._lib.gpry_group_size(self._h, C.byref(n), C.byref(tr))
        self.size, self.transport = n.value, {0: "host", 1: "rccl"}[tr.value]
        self.note = self._lib.gpry_group_last_error(self._h).decode(errors="replace")
        self.sweep_epoch = 0
        self._sweep_M = 0
        self.d = 0

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.gpry_group_last_error(self._h).decode(errors="replace")
            raise GpryHipError(f"{what} failed ({rc}): {msg}")

    def close(self):
        if getattr(self, "_h", None):
            try:
                self._lib.gpry_group_destroy(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    def __del__(self):
        self.close()

    def member(self, i):
        """Member ``i`` as a (non-owning) ``Device`` -- options, timers."""
        h = self._lib.gpry_group_member(self._h, int(i))
        if not h:
            raise IndexError(i)
        v = Device._view(h, self.devices[i])
        v._group = self                # the view must not outlive the group
        return v

    def set_model(self, X_, y_, alpha, kernel_id, theta, affine=None):
        """Replicate (training set, theta, affine maps) on every owned member and factorise there."""
        X_ = _f64(X_)
        N, d = X_.shape
        y_ = _f64(y_, (N,))
        alpha = _f64(np.broadcast_to(alpha, (N,)))
        if int(kernel_id) & KERNEL_WHITE:
            raise NotImplementedError("a device group does not carry the white term (WhiteKernel) of the kernel yet")
        theta = _f64(theta, (d + 1,))
        tf = make_affine(*affine) if affine is not None else None
        info = C.c_int(0)
        self._check(self._lib.gpry_group_set_model(self._h, _ptr(X_), _ptr(y_), _ptr(alpha), N, d, int(kernel_id),
                                                   _ptr(theta), C.byref(tf) if tf is not None else None,
                                                   C.byref(info)), "gpry_group_set_model")
        self.d = d
        return info.value

    def set_gates(self, sv=None, coef=None, gamma=0.0, intercept=0.0, positive_is_finite=True,
                  trust_bounds=None):
        n_sv = 0
        if sv is not None and len(sv):
            sv = _f64(sv)
            n_sv = sv.shape[0]
            coef = _f64(coef, (n_sv,))
        else:
            sv = coef = None
        tb = None if trust_bounds is None else _f64(trust_bounds)
        self._check(self._lib.gpry_group_set_gates(self._h, _ptr(sv), _ptr(coef), n_sv, float(gamma),
                                                   float(intercept), int(bool(positive_is_finite)), _ptr(tb)),
                    "gpry_group_set_gates")

    def sweep_logexp(self, X, zeta, baseline, sigma_n, mask=None, M=None, want=("y", "sigma", "acq"),
                     y_given=None, sigma_given=None):
        if X is not None:
            X = _f64(X)
            M = X.shape[0]
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
        out = {k: (np.empty(M) if k in want else None) for k in ("y", "sigma", "acq")}
        n_nan = C.c_int64(0)
        if y_given is None and sigma_given is None:
            self._check(self._lib.gpry_group_sweep_logexp(
                self._h, _ptr(X), M, _ptr(mask), float(zeta), float(baseline), float(sigma_n),
                _ptr(out["y"]), _ptr(out["sigma"]), _ptr(out["acq"]), C.byref(n_nan)), "gpry_group_sweep_logexp")
        else:
            y_given, sigma_given = _given_arrays(y_given, sigma_given, M)
            self._check(self._lib.gpry_group_sweep_logexp_given(
                self._h, _ptr(X), M, _ptr(mask), _ptr(y_given), _ptr(sigma_given), float(zeta), float(baseline),
                float(sigma_n), _ptr(out["y"]), _ptr(out["sigma"]), _ptr(out["acq"]), C.byref(n_nan)),
                "gpry_group_sweep_logexp_given")
        out["n_nan"] = n_nan.value
        self.sweep_epoch += 1
        self._sweep_M = M
        return out

    def sweep_fetch(self, want=("y", "sigma")):
        M = self._sweep_M
        out = {k: (np.empty(M) if k in want else None) for k in ("y", "sigma", "acq")}
        self._check(self._lib.gpry_group_sweep_fetch(self._h, M, _ptr(out["y"]), _ptr(out["sigma"]),
                                                     _ptr(out["acq"])), "gpry_group_sweep_fetch")
        return out

    def sweep_topk(self, Kp, exclude=None):
        """(records sorted by (acq desc, global idx desc), bound, exhausted)."""
        Kp = int(Kp)
        top = np.zeros(max(Kp, 1) * self.size, dtype=CAND_DTYPE)
        n_out, bound, exh = C.c_int64(0), C.c_double(0.0), C.c_int(0)
        if exclude is not None and len(exclude):
            exclude = np.ascontiguousarray(np.sort(np.asarray(exclude, dtype=np.int64)))
            nex = len(exclude)
        else:
            exclude, nex = None, 0
        self._check(self._lib.gpry_group_sweep_topk(self._h, Kp, _ptr(exclude), nex, _ptr(top), C.byref(n_out),
                                                    C.byref(bound), C.byref(exh)), "gpry_group_sweep_topk")
        return top[:n_out.value], bound.value, bool(exh.value)

    def lml_batch(self, thetas, eval_gradient=True):
        thetas = _f64(np.atleast_2d(thetas))
        n, w = thetas.shape
        lml = np.empty(n)
        grad = np.zeros((n, w)) if eval_gradient else None
        info = np.zeros(n, dtype=np.int32)
        self._check(self._lib.gpry_group_lml_batch(self._h, _ptr(thetas), n, int(bool(eval_gradient)), _ptr(lml),
                                                   _ptr(grad), _ptr(info)), "gpry_group_lml_batch")
        return (lml, grad, info) if eval_gradient else (lml, info)


class RcclComm:
    """RCCL communicator of one rank (one process per GPU)."""

    def __init__(self, dev, world, rank, unique_id):
        self._dev = dev
        self._lib = dev._lib
        self.world, self.rank = int(world), int(rank)
        self._h = C.c_void_p()
        uid = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        dev._check(self._lib.gpry_comm_init(dev._h, self.world, self.rank, _ptr(uid),
                                            C.byref(self._h)), "gpry_comm_init")

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = np.zeros(128, dtype=np.uint8)
        if lib.gpry_comm_unique_id(_ptr(buf)) != 0:
            raise GpryHipError("gpry_comm_unique_id failed: " +
                               lib.gpry_last_error(None).decode(errors="replace"))
        return buf.tobytes()

    def info(self):
        """(ranks, rank, device) as RCCL reports them for this communicator."""
        n, r, dv = C.c_int(0), C.c_int(0), C.c_int(0)
        self._dev._check(self._lib.gpry_comm_info(self._h, C.byref(n), C.byref(r), C.byref(dv)),
                         "gpry_comm_info")
        return n.value, r.value, dv.value

    def allgather(self, arr):
        arr = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + arr.shape, dtype=arr.dtype)
        self._dev._check(self._lib.gpry_comm_allgather(self._h, _ptr(arr), arr.nbytes, _ptr(out)),
                         "gpry_comm_allgather")
        return out

    def allreduce_max(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64).copy()
        self._dev._check(self._lib.gpry_comm_allreduce_max(self._h, _ptr(arr), arr.size),
                         "gpry_comm_allreduce_max")
        return arr

    def barrier(self):
        self._dev._check(self._lib.gpry_comm_barrier(self._h), "gpry_comm_barrier")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpry_comm_destroy(self._h)
            self._h = None
