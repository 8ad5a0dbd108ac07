"""ctypes binding of libbogp.so (include/bogp.h).  There is no fallback: if the library is missing or no
gfx950 device is usable, every entry point raises -- the product path never computes on the CPU."""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Optional, Sequence, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbogp.so")

OK = 0
ERR_INVALID, ERR_HIP, ERR_NOT_POSDEF, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_LLF_POSITIVE = -1, -2, -3, -4, -5, -6
KERNEL_SE, KERNEL_MATERN12, KERNEL_MATERN32, KERNEL_MATERN52, KERNEL_ABSEXP, KERNEL_CUBIC, KERNEL_GENEXP, KERNEL_MATERN_NU = 0, 1, 2, 3, 4, 5, 6, 7
MODE_NOISELESS, MODE_NOISY, MODE_NOISE_ESTIM = 0, 1, 2
ACQ_EI, ACQ_EPSILON_PI, ACQ_UCB, ACQ_MGFI = 0, 1, 2, 3
ACQ_NONE = -1  # BOGP_ACQ_NONE: bogp_sweep_constrained's feasibility-only criterion
TREND_CONSTANT, TREND_LINEAR, TREND_QUADRATIC = 0, 1, 2
SELFTEST_PROFILE, SELFTEST_BESSEL_K, SELFTEST_RGAMMA, SELFTEST_BESSEL_K_PAIRS, SELFTEST_MATERN_NU_PAIRS = range(5)
(CRITERIA_NDTR, CRITERIA_NORM_PDF, CRITERIA_EHVI_G, CRITERIA_ACQ_VALUE, CRITERIA_FEASIBILITY, CRITERIA_ACQ_UPPER_BOUND,
 CRITERIA_ACQ_UPPER_BOUND_INTERVAL, CRITERIA_PRUNE_BELOW) = range(8)  # BOGP_CRITERIA_*: selectors of bogp_selftest_criteria
CRITERIA_COLUMNS = 8
ABI_VERSION = 9  # BOGP_ABI_VERSION of include/bogp.h this binding table was written for
MAX_Q = 64
PRUNE_PATH_NONE, PRUNE_PATH_CHUNKS, PRUNE_PATH_ONEPASS, PRUNE_PATH_ONEPASS_FALLBACK = 0, 1, 2, 3  # bogp_last_prune_path
# bogp_contract_tile_rows: workgroups of the 64-row grid per four CUs from which a launch takes 64 / 32 rows (csrc/bogp_internal.h)
CONTRACT_TILE64_MIN_WG_PER_4CU, CONTRACT_TILE32_MIN_WG_PER_4CU = 14, 6
MAX_TARGETS = 8
MAX_TOPK = 32
MAX_BELIEVED = 32  # BOGP_MAX_BELIEVED: q + pending points of one bogp_sweep_believer call
MAX_PATHS, MAX_FEATURES = 16, 16384  # BOGP_MAX_PATHS / BOGP_MAX_FEATURES: paths and features of one bogp_sweep_thompson call
LIFT_MAX_R, LIFT_MAX_RD = 64, 4096  # BOGP_LIFT_MAX_R / BOGP_LIFT_MAX_RD: reduced dimensions and r x D of a lift
MAX_EHVI_CELLS = 65536  # BOGP_MAX_EHVI_CELLS: cells one bogp_sweep_ehvi call takes
COMM_ID_BYTES = 128
COLUMN_REAL, COLUMN_DISCRETE = 0, 1  # BOGP_COLUMN_*: column kinds of bogp_candidates_generate_mixed
SCALES = {"linear": 0, None: 0, "log": 1, "log10": 2, "logit": 3, "bilog": 4}  # Real.scale (variable.py:43-55)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_int64)

# name -> (restype, argtypes); must list every symbol include/bogp.h declares (tests/test_abi.py checks it)
SIGNATURES = {
    "bogp_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "bogp_destroy": (None, [C.c_void_p]),
    "bogp_last_error": (C.c_char_p, [C.c_void_p]),
    "bogp_abi_version": (C.c_int, []),
    "bogp_set_train": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_int, C.c_int]),
    "bogp_select_target": (C.c_int, [C.c_void_p, C.c_int]),
    "bogp_nll": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, _dp, _dp]),
    "bogp_nll_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, _dp, _dp, _ip]),
    "bogp_mle_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, C.c_int, C.c_int, C.c_double,
                                 C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _ip]),
    "bogp_lbfgsb_minimize": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       _dp, _ip, _ip, _ip]),
    "bogp_commit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, _dp]),
    "bogp_nll_restricted": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, _dp, _dp]),
    "bogp_get_state": (C.c_int, [C.c_void_p] + [_dp] * 10),
    "bogp_trend_size": (C.c_int, [C.c_int, C.c_int]),
    "bogp_set_trend_beta": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "bogp_get_trend_state": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp]),
    "bogp_candidates_upload": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "bogp_candidates_upload_lazy": (C.c_int, [C.c_void_p, _dp, C.c_int64]),
    "bogp_candidates_bind": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "bogp_candidates_generate": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int64, C.c_uint64, C.c_int64]),
    "bogp_candidates_generate_lhs": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int64, C.c_uint64, C.c_int64, C.c_int64]),
    "bogp_candidates_generate_lhs_maximin": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int64, C.c_uint64, C.c_int, _dp, _ip]),
    "bogp_candidates_min_pdist2": (C.c_int, [C.c_void_p, _dp]),
    "bogp_candidates_generate_sobol": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), C.c_int]),
    "bogp_candidates_read": (C.c_int, [C.c_void_p, _lp, C.c_int, _dp]),
    "bogp_candidates_set_transform": (C.c_int, [C.c_void_p, _ip, _ip, _dp, _dp]),
    "bogp_predict": (C.c_int, [C.c_void_p, _dp, _dp]),
    "bogp_sweep": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, _dp, _lp, _dp]),
    "bogp_sweep_topk": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _lp]),
    "bogp_sweep_ehvi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp]),
    "bogp_feasibility": (C.c_double, [C.c_double] * 5),
    "bogp_sweep_constrained": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp, _dp]),
    "bogp_sweep_ehvi_constrained": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp, _dp]),
    "bogp_sweep_believer": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp, _dp]),
    "bogp_believer_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _ip]),
    "bogp_sweep_thompson": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _lp, _dp, _dp, _dp]),
    "bogp_thompson_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _ip]),
    "bogp_sweep_thompson_constrained": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp]),
    "bogp_thompson_constrained_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _ip]),
    "bogp_ehvi_grid_cells": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int64]),
    "bogp_sweep_believer_ehvi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp, _ip,
                                           _dp, _dp]),
    "bogp_believer_ehvi_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _ip]),
    "bogp_sweep_believer_constrained": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int,
                                                  _dp, _lp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bogp_believer_constrained_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _ip]),
    "bogp_sweep_believer_ehvi_constrained": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp,
                                                       C.c_int, _dp, _lp, _dp, _dp, _dp, _ip, _dp, _dp, _dp]),
    "bogp_believer_ehvi_constrained_last": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _ip]),
    "bogp_lift_set": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "bogp_lift_clear": (C.c_int, [C.c_void_p]),
    "bogp_lift_sweep_topk": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _lp, _lp, _dp, _dp]),
    "bogp_lift_last": (C.c_int, [C.c_void_p, _lp, _dp, _dp]),
    "bogp_forest_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _lp, _ip, _dp, _ip, _ip, _dp, _ip]),
    "bogp_forest_predict": (C.c_int, [C.c_void_p, _dp, _dp]),
    "bogp_forest_leaves": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _dp]),
    "bogp_forest_sweep_topk": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _lp, _dp]),
    "bogp_forest_info": (C.c_int, [C.c_void_p, _lp]),
    "bogp_forest_set_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _lp, _ip, _dp, _ip, _ip, _dp, _ip]),
    "bogp_forest_outputs": (C.c_int, [C.c_void_p]),
    "bogp_forest_predict_multi": (C.c_int, [C.c_void_p, _dp, _dp]),
    "bogp_forest_leaves_multi": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, _dp]),
    "bogp_forest_sweep_ehvi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _lp, _dp, _dp, _dp]),
    "bogp_candidates_generate_mixed": (C.c_int, [C.c_void_p, _ip, _dp, _dp, _ip, C.c_int64, C.c_uint64, C.c_int64]),
    "bogp_gradient": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "bogp_gradient_batch": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp]),
    "bogp_hessian": (C.c_int, [C.c_void_p, _dp, _dp]),
    "bogp_prior_corr": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp]),
    "bogp_point_eval": (C.c_int, [C.c_void_p, _dp, C.c_int, _ip, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "bogp_point_eval_batch": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _ip, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bogp_polish": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double,
                              C.c_double, _dp, _dp, _ip]),
    "bogp_point_eval_ehvi": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bogp_polish_ehvi": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_double,
                                   _dp, _dp, _ip]),
    "bogp_feasibility_grad": (C.c_int, [C.c_double] * 5 + [_dp]),
    "bogp_point_eval_constrained": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _dp,
                                              _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bogp_polish_constrained": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _dp, _dp,
                                          C.c_int, C.c_double, C.c_double, _dp, _dp, _ip]),
    "bogp_point_eval_ehvi_constrained": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp,
                                                   _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "bogp_polish_ehvi_constrained": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp,
                                               C.c_int, C.c_double, C.c_double, _dp, _dp, _ip]),
    "bogp_comm_unique_id": (C.c_int, [C.c_char_p]),
    "bogp_comm_init": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "bogp_comm_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bogp_comm_info": (C.c_int, [C.c_void_p, _ip, _ip]),
    "bogp_comm_destroy": (C.c_int, [C.c_void_p]),
    "bogp_exchange_argmax": (C.c_int, [C.c_void_p, C.c_int64, _dp, _lp, _dp]),
    "bogp_exchange_topk": (C.c_int, [C.c_void_p, C.c_int64, _dp, _lp, _dp]),
    "bogp_reduce_pairs": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _lp, _dp]),
    "bogp_merge_topk": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _lp, _dp]),
    "bogp_last_timing": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _ip]),
    "bogp_set_prune": (C.c_int, [C.c_void_p, C.c_int]),
    "bogp_last_contracted_rows": (C.c_int, [C.c_void_p, _lp]),
    "bogp_last_prune_path": (C.c_int, [C.c_void_p, _ip, _lp, _ip]),
    "bogp_prune_decide": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "bogp_set_contract_tile": (C.c_int, [C.c_void_p, C.c_int]),
    "bogp_last_contract_tile": (C.c_int, [C.c_void_p, _ip]),
    "bogp_contract_tile_rows": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "bogp_sweep_chunk_rows": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "bogp_acq_upper_bound": (C.c_double, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bogp_prune_below": (C.c_int, [C.c_double, C.c_double]),
    "bogp_set_prune_bound32": (C.c_int, [C.c_void_p, C.c_int]),
    "bogp_last_bound32": (C.c_int, [C.c_void_p, _lp, _lp, _ip]),
    "bogp_debug_bound32": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, C.POINTER(C.c_ubyte), _lp]),
    "bogp_debug_live": (None, [_lp, _lp, _lp]),
    "bogp_bound32_margin": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp]),
    "bogp_acq_upper_bound_interval": (C.c_double, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bogp_flops_per_candidate": (C.c_double, [C.c_void_p]),
    "bogp_nll_path": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bogp_chol_wide_panels": (C.c_int, [C.c_int, _ip, C.c_int]),
    "bogp_selftest_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, _dp, C.c_int64, _dp]),
    "bogp_selftest_criteria": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int64, _dp]),
    "bogp_selftest_feasibility_grad": (C.c_int, [C.c_void_p, _dp, C.c_int64, _dp]),
    "bogp_selftest_gemm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _dp, C.c_int, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_int]),
}

_lib = None


class BogpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libbogp error %d: %s" % (code, msg))
        self.code = code


class NotPositiveDefinite(BogpError, np.linalg.LinAlgError):
    """Cholesky info > 0 (or llf > 0, which the reference also rejects): the host maps it to llf = -inf."""


def load():
    """dlopen libbogp.so and bind every symbol.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libbogp.so not found at %s -- build it with `python __graft_entry__.py` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH
        )
    # Load order matters: the PyTorch wheel bundles its own libamdhip64 (the only ROCm library libbogp.so needs; it links
    # no BLAS) with the SAME soname as /opt/rocm's.  The dynamic loader keeps whichever copy comes first, and torch
    # crashes when it is handed the system copy; the other way round (libbogp on torch's copy) works.  So torch goes
    # first whenever it is installed (it provides torch.distributed for the multi-GPU exchange anyway).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table drift apart
        fn.restype = res
        fn.argtypes = args
    if lib.bogp_abi_version() != ABI_VERSION:
        raise ImportError("libbogp.so is at ABI %d, this binding at %d: rebuild it (make -C %s)"
                          % (lib.bogp_abi_version(), ABI_VERSION, os.path.join(os.path.dirname(LIB_PATH), "csrc")))
    _lib = lib
    return lib


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_dp)


def _pack_acq(acq: Sequence[Tuple[int, float]]) -> Tuple[np.ndarray, np.ndarray]:
    """(ids int32 (q,), pars float64 (q,)) of q criteria; a parameter of None is 0."""
    return np.ascontiguousarray([a for a, _ in acq], dtype=np.int32), _f64([float(p) if p is not None else 0.0 for _, p in acq])


def feasibility(mu: float, mse: float, sigma2: float, lo: float, hi: float) -> float:
    """P(lo <= Y <= hi) for Y ~ N(mu, mse) as the constrained sweep forms it (bogp_feasibility: the indicator under EI's
    small-variance guard, else the difference of two normal cdfs taken in the tail the interval lies in).  No device is touched."""
    return float(load().bogp_feasibility(float(mu), float(mse), float(sigma2), float(lo), float(hi)))


def feasibility_grad(mu: float, mse: float, sigma2: float, lo: float, hi: float) -> Tuple[float, float, float]:
    """(F, dF/dmu, dF/dsd) of `feasibility` in the posterior's mean and standard deviation (bogp_feasibility_grad): F has the bits of
    `feasibility`; both derivatives are exactly 0 under the small-variance guard, and an infinite side contributes exactly 0.  No
    device is touched."""
    out = np.empty(3)
    if load().bogp_feasibility_grad(float(mu), float(mse), float(sigma2), float(lo), float(hi), _ptr(out)):
        raise BogpError(ERR_INVALID, "bogp_feasibility_grad refused its arguments")
    return float(out[0]), float(out[1]), float(out[2])


def grid_cells(Y, ref_point):
    """(lower, upper), each C x m: libbogp's grid decomposition of the region above `ref_point` that the front of Y (n x m, may
    be empty) does not dominate (bogp_ehvi_grid_cells: `pareto.hypercell_bounds` restated on the host side of the library, the
    same arrays bit for bit).  No device is touched.  ValueError for what the library refuses (m outside [2, MAX_TARGETS], a
    non-finite input, more than MAX_EHVI_CELLS cells)."""
    lib = load()
    r = _f64(ref_point).ravel()
    m = len(r)
    Y = _f64(Y).reshape(-1, m) if np.size(Y) else np.empty((0, m))
    n = lib.bogp_ehvi_grid_cells(m, len(Y), _ptr(Y), _ptr(r), None, None, 0)
    if n < 0:
        raise ValueError("bogp_ehvi_grid_cells refused a front of %d rows in %d objectives (non-finite input, m outside [2, %d] or "
                         "more than %d cells)" % (len(Y), m, MAX_TARGETS, MAX_EHVI_CELLS))  # fmt: skip
    lower, upper = np.empty((n, m)), np.empty((n, m))
    if lib.bogp_ehvi_grid_cells(m, len(Y), _ptr(Y), _ptr(r), _ptr(lower), _ptr(upper), n) != n:
        raise BogpError(ERR_INVALID, "bogp_ehvi_grid_cells: the count changed between two calls")
    return lower, upper


OBJECTIVE_FN = C.CFUNCTYPE(None, _dp, C.c_int, _dp, _dp, C.c_void_p)


def lbfgsb_minimize(fun, x0, bounds, m=10, factr=1e7, pgtol=1e-5, maxfun=15000, maxiter=15000):
    """libbogp's L-BFGS-B (csrc/bogp_lbfgsb.h, the optimiser of the lock-step MLE) on a Python objective `fun(x) -> (f, g)`:
    the counterpart of scipy.optimize.fmin_l_bfgs_b(fun, x0, bounds=bounds) for tests.  No device is touched.
    Returns (x, f, {"funcalls", "nit", "status"})."""
    lib = load()
    x = np.array(x0, dtype=np.float64).ravel()
    n = len(x)
    b = np.asarray(bounds, dtype=np.float64).reshape(n, 2)
    lo, hi = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])

    def cb(xp, nn, fp, gp, _user):
        xv = np.ctypeslib.as_array(xp, shape=(nn,)).copy()
        f, g = fun(xv)
        fp[0] = float(f)
        gv = np.asarray(g, dtype=np.float64).ravel()
        for i in range(nn):
            gp[i] = gv[i]

    cfn = OBJECTIVE_FN(cb)
    f, nfev, nit, status = C.c_double(), C.c_int(), C.c_int(), C.c_int()
    rc = lib.bogp_lbfgsb_minimize(n, int(m), _ptr(x), _ptr(lo), _ptr(hi), float(factr), float(pgtol), int(maxfun), int(maxiter),
                                  C.cast(cfn, C.c_void_p), None, C.byref(f), C.byref(nfev), C.byref(nit), C.byref(status))
    if rc != OK:
        raise BogpError(rc, "bogp_lbfgsb_minimize: invalid arguments")
    return x, f.value, {"funcalls": nfev.value, "nit": nit.value, "status": status.value}


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through libbogp (call on ONE rank, distribute the 128 bytes to the others)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().bogp_comm_unique_id(buf)
    if rc != OK:
        raise BogpError(rc, "bogp_comm_unique_id failed (librccl missing?)")
    return buf.raw


def reduce_pairs_c(gathered: np.ndarray):
    """bogp_reduce_pairs on host records (R, q, 2 + d): (values (q,), global indices (q,), points (q, d) or None)."""
    g = _f64(gathered)
    R, q, rec = g.shape
    d = rec - 2
    val, idx = np.empty(q), np.empty(q, dtype=np.int64)
    x = np.empty((q, d)) if d else None
    rc = load().bogp_reduce_pairs(R, q, d, _ptr(g), _ptr(val), idx.ctypes.data_as(_lp), _ptr(x))
    if rc != OK:
        raise BogpError(rc, "bogp_reduce_pairs: invalid arguments")
    return val, idx, x


def merge_topk_c(gathered: np.ndarray):
    """bogp_merge_topk on host records (R, q, k, 2 + d): (values (q, k), global indices (q, k), points (q, k, d) or None)."""
    g = _f64(gathered)
    R, q, k, rec = g.shape
    d = rec - 2
    val, idx = np.empty((q, k)), np.empty((q, k), dtype=np.int64)
    x = np.empty((q, k, d)) if d else None
    rc = load().bogp_merge_topk(R, q, k, d, _ptr(g), _ptr(val), idx.ctypes.data_as(_lp), _ptr(x))
    if rc != OK:
        raise BogpError(rc, "bogp_merge_topk: invalid arguments")
    return val, idx, x


def debug_live():
    """bogp_debug_live: (live device + mapped pinned allocations, their bytes, live events) held by the handles of this process."""
    a, b, e = C.c_int64(), C.c_int64(), C.c_int64()
    load().bogp_debug_live(C.byref(a), C.byref(b), C.byref(e))
    return int(a.value), int(b.value), int(e.value)


def trend_size_of(trend: int, d: int) -> int:
    """Columns of the trend basis (bogp_trend_size; needs no device)."""
    return 1 if trend == TREND_CONSTANT else (d + 1 if trend == TREND_LINEAR else (d + 1) * (d + 2) // 2)


@functools.lru_cache(maxsize=32)
def sobol_direction_numbers(d: int, bits: int = 30) -> np.ndarray:
    """(Cached per (d, bits): building the table costs 30 scipy engines, and generate_candidates(method="sobol") asks for it on
    every ask().  Needs scipy >= 1.9 for the `bits=` keyword of `qmc.Sobol`.  The returned array is shared: do not write to it.)
    The (d, bits) direction numbers of scipy's unscrambled Sobol' generator (Joe & Kuo tables): what the reference's
    `sobol_seq` call resolves to in this image.  Data for `bogp_candidates_generate_sobol`, which
    carries no table of its own.  Recovered through scipy's PUBLIC interface only: point n of the sequence is the XOR of
    the direction numbers over the set bits of the Gray code of n, and gray(2^b) = 2^b ^ 2^(b-1), so
    sv[b] = x_(2^b) ^ sv[b-1] with x_(2^b) read off `Sobol.fast_forward(2^b).random(1)` (exact multiples of 2^-bits)."""
    from scipy.stats import qmc

    sv = np.zeros((int(d), int(bits)), dtype=np.uint64)
    prev = np.zeros(int(d), dtype=np.uint64)
    for b in range(int(bits)):
        eng = qmc.Sobol(d=int(d), scramble=False, bits=int(bits))
        if b:
            eng.fast_forward(2**b)
        else:
            eng.fast_forward(1)
        ints = np.round(eng.random(1)[0] * 2.0 ** int(bits)).astype(np.uint64)
        sv[:, b] = ints ^ prev if b else ints
        prev = sv[:, b]
    return np.ascontiguousarray(sv)


class Engine:
    """One handle = one GPU.  Thin, stateful wrapper over the C ABI; raises BogpError on any non-zero code."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.bogp_create(int(device), C.byref(h))
        if rc != OK:
            raise BogpError(rc, (self._lib.bogp_last_error(None) or b"").decode())
        self._h = h
        self.device = int(device)
        self.N = self.d = 0
        self.trend, self.estimate_trend = TREND_CONSTANT, False
        self.M = 0
        self.comm_rank, self.comm_world = 0, 0  # world > 0 once a communicator is set (comm_init / comm_attach)
        self._keep = None  # keeps bound device memory owners alive

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bogp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc == OK:
            return
        msg = (self._lib.bogp_last_error(self._h) or b"").decode()
        if rc in (ERR_NOT_POSDEF, ERR_LLF_POSITIVE):
            raise NotPositiveDefinite(rc, msg)
        raise BogpError(rc, msg)

    # -- training set / likelihood / commit ---------------------------------------------------------
    def set_train(self, X, y):
        X = _f64(X)
        y = _f64(y).reshape(len(X), -1)
        self._check(self._lib.bogp_set_train(self._h, _ptr(X), _ptr(y), X.shape[0], X.shape[1], y.shape[1]))
        self.N, self.d = X.shape
        self.n_t = y.shape[1]

    def select_target(self, t: int):
        """Column of a multi-target y that get_state / predict / sweep / gradient work on (0 after set_train, commit)."""
        self._check(self._lib.bogp_select_target(self._h, int(t)))

    def _trend_beta(self, trend, estimate_trend, beta) -> float:
        """Fixed coefficients of a p > 1 basis travel through bogp_set_trend_beta; the scalar argument serves p = 1."""
        if trend == TREND_CONSTANT:
            return float(np.ravel(beta)[0]) if np.ndim(beta) else float(beta)
        if not estimate_trend:
            b = _f64(beta).ravel()
            self._check(self._lib.bogp_set_trend_beta(self._h, _ptr(b), len(b)))
        return 0.0

    def nll(self, kernel, mode, par, noise_var=0.0, estimate_trend=False, beta=0.0, eval_grad=False, trend=TREND_CONSTANT):
        """log-likelihood (and d llf / d par) at `par`; raises NotPositiveDefinite where the reference returns -inf."""
        par = _f64(par).ravel()
        llf = C.c_double()
        grad = np.zeros(len(par)) if eval_grad else None
        b = self._trend_beta(trend, estimate_trend, beta)
        self._check(
            self._lib.bogp_nll(self._h, kernel, mode, _ptr(par), len(par), float(noise_var), int(trend),
                               int(bool(estimate_trend)), b, C.byref(llf), _ptr(grad))
        )  # fmt: skip
        return (llf.value, grad) if eval_grad else llf.value

    def nll_batch(self, kernel, mode, pars, noise_var=0.0, estimate_trend=False, beta=0.0, eval_grad=False, trend=TREND_CONSTANT):
        """P likelihood (+ gradient) evaluations in one device round trip: `pars` is (P, n_par).  Returns (llf (P,), grad (P, n_par)
        or None, info (P,) int32): llf[s] = -inf where the reference returns -inf (info[s] = ERR_NOT_POSDEF / ERR_LLF_POSITIVE /
        ERR_INVALID), with a zero gradient row.  Slot s holds the bits of the s-th sequential `nll` call."""
        pars = _f64(pars)
        if pars.ndim != 2:
            raise ValueError("pars must be (P, n_par)")
        P, n_par = pars.shape
        llf = np.empty(P)
        grad = np.zeros((P, n_par)) if eval_grad else None
        info = np.zeros(P, dtype=np.int32)
        b = self._trend_beta(trend, estimate_trend, beta)
        self._check(
            self._lib.bogp_nll_batch(self._h, kernel, mode, P, _ptr(pars), n_par, float(noise_var), int(trend),
                                     int(bool(estimate_trend)), b, _ptr(llf), _ptr(grad), info.ctypes.data_as(_ip))
        )  # fmt: skip
        llf[info != OK] = -np.inf
        return llf, grad, info

    def mle_batch(self, kernel, mode, x0, lo, hi, noise_var=0.0, estimate_trend=False, beta=0.0, trend=TREND_CONSTANT, restricted=False,
                  eval_budget=0, m=10, factr=1e7, pgtol=1e-5, chain_rule=False, prune_reserve=0):
        """The R restarts of the MLE in lock step (bogp_mle_batch): x0 (R, n_par) log10 starts, lo / hi (n_par,) log10 bounds.
        `prune_reserve` > 0 stops the worst run whenever fewer than that many evaluations per active run remain of a shared budget.
        `chain_rule=True` hands the optimiser the gradient w.r.t. log10(par) instead of the reference's un-scaled one (an extension).
        Returns (xopt (R, n_par) log10, fopt (R,) = -llf, n_evals (R,), status (R,), rounds)."""
        x0 = _f64(x0)
        if x0.ndim != 2:
            raise ValueError("x0 must be (R, n_par)")
        R, n_par = x0.shape
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if len(lo) != n_par or len(hi) != n_par:
            raise ValueError("bounds must have n_par entries")
        xopt, fopt = np.empty((R, n_par)), np.empty(R)
        nev, status = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
        rounds = C.c_int()
        b = self._trend_beta(trend, estimate_trend, beta)
        self._check(
            self._lib.bogp_mle_batch(self._h, kernel, mode, int(bool(restricted)), R, _ptr(x0), n_par, _ptr(lo), _ptr(hi), float(noise_var),
                                     int(trend), int(bool(estimate_trend)), b, int(eval_budget), int(m), float(factr), float(pgtol),
                                     1 if chain_rule else 0, int(prune_reserve), _ptr(xopt), _ptr(fopt), nev.ctypes.data_as(_ip), status.ctypes.data_as(_ip), C.byref(rounds))
        )  # fmt: skip
        return xopt, fopt, nev, status, rounds.value

    def nll_restricted(self, kernel, mode, par, noise_var=0.0, estimate_trend=False, beta=0.0, eval_grad=False, trend=TREND_CONSTANT):
        """Restricted (REML) log-likelihood, gpr.py:813-918.  exp(llf) > 1 gives -inf WITH the gradient of the finite
        value, as the reference returns it; a failed factorisation raises NotPositiveDefinite."""
        par = _f64(par).ravel()
        llf = C.c_double()
        grad = np.zeros(len(par)) if eval_grad else None
        b = self._trend_beta(trend, estimate_trend, beta)
        rc = self._lib.bogp_nll_restricted(self._h, kernel, mode, _ptr(par), len(par), float(noise_var), int(trend),
                                           int(bool(estimate_trend)), b, C.byref(llf), _ptr(grad))  # fmt: skip
        if rc == ERR_LLF_POSITIVE:
            return (-np.inf, grad) if eval_grad else -np.inf
        self._check(rc)
        return (llf.value, grad) if eval_grad else llf.value

    def commit(self, kernel, mode, par, noise_var=0.0, estimate_trend=False, beta=0.0, trend=TREND_CONSTANT) -> float:
        par = _f64(par).ravel()
        llf = C.c_double()
        b = self._trend_beta(trend, estimate_trend, beta)
        self._check(
            self._lib.bogp_commit(self._h, kernel, mode, _ptr(par), len(par), float(noise_var), int(trend),
                                  int(bool(estimate_trend)), b, C.byref(llf))
        )  # fmt: skip
        self.trend = int(trend)
        self.estimate_trend = bool(estimate_trend)
        return llf.value

    def trend_size(self, trend=None) -> int:
        return int(self._lib.bogp_trend_size(int(self.trend if trend is None else trend), int(self.d)))

    def get_state(self, with_C=True) -> dict:
        if getattr(self, "n_t", 1) > 1:  # one column per target: gamma, rho, Yt (N, n_t); sigma2, noise_var (n_t,)
            cols = []
            for t in range(self.n_t):
                self.select_target(t)
                cols.append(self._get_state_active(with_C and t == 0))
            self.select_target(0)
            out = dict(cols[0])
            for k in ("gamma", "rho", "Yt"):
                out[k] = np.column_stack([c[k] for c in cols])
            out["sigma2"] = np.array([c["sigma2"] for c in cols])
            out["noise_var"] = np.array([c["noise_var"] for c in cols])
            return out
        return self._get_state_active(with_C)

    def _get_state_active(self, with_C=True) -> dict:
        N = self.N
        Cm = np.empty((N, N)) if with_C else None
        v = {k: np.zeros(N) for k in ("gamma", "rho", "Yt", "Ft", "Q")}
        s = [C.c_double() for _ in range(4)]
        self._check(
            self._lib.bogp_get_state(self._h, _ptr(Cm), _ptr(v["gamma"]), _ptr(v["rho"]), _ptr(v["Yt"]), _ptr(v["Ft"]),
                                     _ptr(v["Q"]), *[C.cast(C.byref(x), _dp) for x in s])
        )  # fmt: skip
        out = dict(v, G=s[0].value, beta=s[1].value, sigma2=s[2].value, noise_var=s[3].value)
        if with_C:
            out["C"] = Cm
        if getattr(self, "trend", TREND_CONSTANT) != TREND_CONSTANT:  # p > 1: Ft, Q (N, p), G (p, p), beta (p,)
            p = self.trend_size()
            est = getattr(self, "estimate_trend", False)
            Ft, Q, G, beta = np.zeros((N, p)), np.zeros((N, p)), np.zeros((p, p)), np.zeros(p)
            self._check(self._lib.bogp_get_trend_state(self._h, _ptr(Ft) if est else None, _ptr(Q) if est else None,
                                                       _ptr(G) if est else None, _ptr(beta)))  # fmt: skip
            out.update(Ft=Ft, Q=Q, G=G, beta=beta)
        return out

    # -- candidates ---------------------------------------------------------------------------------
    def upload_candidates(self, Xs, lazy=False):
        """Host candidates (M, d).  `lazy=True`: only the head is copied now, the rest travels chunk by chunk beside the kernels of the
        NEXT predict / sweep / sweep_topk call (bogp_candidates_upload_lazy) -- the array is kept alive by the engine until then, and
        the caller must not modify it before that call returns."""
        Xs = _f64(Xs)
        if Xs.ndim != 2 or Xs.shape[1] != self.d:
            raise ValueError("candidates must have shape (M, %d)" % self.d)
        fn = self._lib.bogp_candidates_upload_lazy if lazy else self._lib.bogp_candidates_upload
        self._check(fn(self._h, _ptr(Xs), Xs.shape[0]))
        self.M = Xs.shape[0]
        self._last_q, self._last_topk = -1, (-1, -1)  # winners of an earlier sweep refer to other rows
        self._keep = Xs if lazy else None

    def bind_candidates(self, device_ptr: int, M: int, owner=None):
        """Adopt caller-owned device memory (M x d float64 row-major), e.g. a torch tensor's data_ptr()."""
        self._check(self._lib.bogp_candidates_bind(self._h, C.c_void_p(int(device_ptr)), int(M)))
        self.M = int(M)
        self._last_q, self._last_topk = -1, (-1, -1)
        self._keep = owner

    def generate_candidates(self, lo, hi, M: int, seed: int = 0, first_row: int = 0, method: str = "uniform",
                            n_total: Optional[int] = None, sobol_sv: Optional[np.ndarray] = None, maximin: int = 5):
        """M points in the box [lo, hi] drawn ON the device -- no host sampling, no H2D copy.  `method` follows
        RealSpace._sample (search_space.py:742-754): "uniform" (Philox4x32-10 stream `seed`, rows [first_row,
        first_row + M)); "LHS" (rows [first_row, first_row + M) of an `n_total`-point Latin hypercube, default M);
        "sobol" (points first_row + 1 ... of the unscrambled sequence -- the reference skips point 0 -- for the
        direction numbers `sobol_sv` (d x bits), default scipy's); "LHS-maximin" (the best of `maximin` hypercubes by
        minimum pairwise distance, pyDOE's criterion; (distance, trial) left in `self.last_maximin`)."""
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if len(lo) != self.d or len(hi) != self.d:
            raise ValueError("bounds must have %d entries" % self.d)
        useed = C.c_uint64(int(seed) & (2**64 - 1))
        if method == "uniform":
            rc = self._lib.bogp_candidates_generate(self._h, _ptr(lo), _ptr(hi), int(M), useed, int(first_row))
        elif method == "LHS":
            n_total = int(M) + int(first_row) if n_total is None else int(n_total)
            rc = self._lib.bogp_candidates_generate_lhs(self._h, _ptr(lo), _ptr(hi), int(M), useed, int(first_row), n_total)
        elif method == "LHS-maximin":  # pyDOE's criterion="maximin": the reference's own "LHS" (search_space.py:751)
            if int(first_row) != 0 or (n_total is not None and int(n_total) != int(M)):
                raise NotImplementedError("the maximin criterion needs the whole design on one device (no row shards)")
            dist, it = C.c_double(), C.c_int()
            rc = self._lib.bogp_candidates_generate_lhs_maximin(self._h, _ptr(lo), _ptr(hi), int(M), useed, int(maximin),
                                                                 C.cast(C.byref(dist), _dp), C.cast(C.byref(it), _ip))  # fmt: skip
            self.last_maximin = (dist.value, it.value)
        elif method == "sobol":
            sv = sobol_direction_numbers(self.d) if sobol_sv is None else sobol_sv
            sv = np.ascontiguousarray(sv, dtype=np.uint64)
            if sv.ndim != 2 or sv.shape[0] != self.d:
                raise ValueError("sobol_sv must be (d, bits)")
            rc = self._lib.bogp_candidates_generate_sobol(self._h, _ptr(lo), _ptr(hi), int(M), int(first_row) + 1,
                                                          sv.ctypes.data_as(C.POINTER(C.c_uint64)), int(sv.shape[1]))  # fmt: skip
        else:
            raise ValueError("method must be 'uniform', 'LHS' or 'sobol'")
        self._check(rc)
        self.M = int(M)
        self._last_q, self._last_topk = -1, (-1, -1)
        self._keep = None

    def set_candidate_transform(self, scales=None, precisions=None, lo=None, hi=None):
        """Post-processing of device-generated candidates as RealSpace._sample does it (search_space.py:754): `scales` per
        dimension ("linear" | "log" | "log10" | "logit" | "bilog": the design is drawn in the transformed box and mapped
        back), `precisions` (decimals or None) with the variables' own bounds `lo`, `hi` for the clip.  No arguments:
        plain designs again."""
        if scales is None and precisions is None:
            self._check(self._lib.bogp_candidates_set_transform(self._h, None, None, None, None))
            return
        d = self.d
        sc = np.ascontiguousarray([SCALES[s] for s in (scales if scales is not None else [None] * d)], dtype=np.int32)
        pr = np.ascontiguousarray([-1 if p is None else int(p) for p in (precisions if precisions is not None else [None] * d)], dtype=np.int32)
        if len(sc) != d or len(pr) != d:
            raise ValueError("scales / precisions must have %d entries" % d)
        lo_ = _f64(lo).ravel() if lo is not None else None
        hi_ = _f64(hi).ravel() if hi is not None else None
        self._check(self._lib.bogp_candidates_set_transform(self._h, sc.ctypes.data_as(_ip), pr.ctypes.data_as(_ip), _ptr(lo_), _ptr(hi_)))

    def min_pairwise_distance(self) -> float:
        """min over pairs of the Euclidean distance between the current candidates (scipy's pdist(...).min())."""
        out = C.c_double()
        self._check(self._lib.bogp_candidates_min_pdist2(self._h, C.cast(C.byref(out), _dp)))
        return float(np.sqrt(out.value))

    def read_candidates(self, rows) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        out = np.empty((len(rows), self.d))
        self._check(self._lib.bogp_candidates_read(self._h, rows.ctypes.data_as(_lp), len(rows), _ptr(out)))
        return out

    # -- posterior / sweep ----------------------------------------------------------------------------
    def predict(self, eval_MSE=True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        mu = np.empty(self.M)
        mse = np.empty(self.M) if eval_MSE else None
        self._check(self._lib.bogp_predict(self._h, _ptr(mu), _ptr(mse)))
        return mu, mse

    def sweep(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize=True, return_values=False, local_result=True):
        """Posterior + q criteria + argmax over the current candidates: (best_val (q,), best_idx (q,)[, values (q, M)]).
        local_result=False only queues the sweep (no host wait, returns None): its winners stay on the device for the
        exchange_argmax() call that follows."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        self._last_q, self._last_topk = -1, (-1, -1)
        if not local_result:
            self._check(self._lib.bogp_sweep(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                             None, None, None))  # fmt: skip
            self._last_q = q
            return None
        best = np.empty(q)
        idx = np.empty(q, dtype=np.int64)
        vals = np.empty((q, self.M)) if return_values else None
        self._check(
            self._lib.bogp_sweep(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                 _ptr(best), idx.ctypes.data_as(_lp), _ptr(vals))
        )  # fmt: skip
        self._last_q = q
        return (best, idx, vals) if return_values else (best, idx)

    def sweep_topk(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize=True, k: int = 1):
        """k best candidates per criterion: (values (q, k), indices (q, k)); rank 0 is the argmax."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        best = np.empty((q, k))
        idx = np.empty((q, k), dtype=np.int64)
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(
            self._lib.bogp_sweep_topk(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                      int(k), _ptr(best), idx.ctypes.data_as(_lp))
        )  # fmt: skip
        self._last_topk = (q, int(k))
        return best, idx

    def sweep_ehvi(self, lower, upper, k: int = 1, return_values=False, return_moments=False):
        """Expected hypervolume improvement of the committed multi-target model over the current candidates, for the
        cells (lower, upper) (C x m each; upper may hold +inf): (best_val (k,), best_idx (k,)[, values (M,)][, mu (M, m),
        mse (M, m)]); rank 0 is the argmax, slots beyond M are (-inf, -1)."""
        lower = _f64(lower)
        upper = _f64(upper)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError("cell bounds must be two C x m arrays of one shape")
        C_, m = lower.shape
        best = np.empty(int(k))
        idx = np.empty(int(k), dtype=np.int64)
        vals = np.empty(self.M) if return_values else None
        mu = np.empty((self.M, m)) if return_moments else None
        mse = np.empty((self.M, m)) if return_moments else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(self._lib.bogp_sweep_ehvi(self._h, int(m), int(C_), _ptr(lower), _ptr(upper), int(k), _ptr(best),
                                              idx.ctypes.data_as(_lp), _ptr(vals), _ptr(mu), _ptr(mse)))  # fmt: skip
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out

    def sweep_constrained(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize, lo, hi, k: int = 1, return_values=False,
                          return_pof=False, return_moments=False):
        """q feasibility-weighted criteria of the committed multi-target model over the current candidates (bogp_sweep_constrained):
        target 0 is the objective, target j the constraint feasible in [lo[j - 1], hi[j - 1]] (either side may be infinite); value =
        criterion on target 0 (EI, EpsilonPI, MGFI; ACQ_NONE: 1) x the product of the constraints' probabilities of feasibility.
        Returns (best_val (q, k), best_idx (q, k)[, values (q, M)][, pof (M,)][, mu (M, m), mse (M, m)]); rank 0 is the argmax, slots
        beyond M are (-inf, -1)."""
        q, k = len(acq), int(k)
        ids, pars = _pack_acq(acq)
        lo, hi = self._constraint_bounds(lo, hi)
        m = len(lo) + 1
        best = np.empty((q, k))
        idx = np.empty((q, k), dtype=np.int64)
        vals = np.empty((q, self.M)) if return_values else None
        pof = np.empty(self.M) if return_pof else None
        mu = np.empty((self.M, m)) if return_moments else None
        mse = np.empty((self.M, m)) if return_moments else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(self._lib.bogp_sweep_constrained(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                                     len(lo), _ptr(lo), _ptr(hi), k, _ptr(best), idx.ctypes.data_as(_lp), _ptr(vals),
                                                     _ptr(pof), _ptr(mu), _ptr(mse)))  # fmt: skip
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_pof:
            out += (pof,)
        if return_moments:
            out += (mu, mse)
        return out

    def sweep_ehvi_constrained(self, lower, upper, lo, hi, k: int = 1, return_values=False, return_pof=False, return_moments=False):
        """Feasibility-weighted EHVI of the committed multi-target model over the current candidates (bogp_sweep_ehvi_constrained):
        targets 0 .. m - 1 are the objectives of the cells (lower, upper) (C x m each, as `sweep_ehvi` takes them; two empty (0, m) arrays
        give the probability of feasibility alone), target m + j the constraint feasible in [lo[j], hi[j]] (either side
        may be infinite); value = EHVI x the product of the constraints' probabilities of feasibility P, and +0.0 where P == 0.
        Returns (best_val (k,), best_idx (k,)[, values (M,)][, pof (M,)][, mu (M, m + c), mse (M, m + c)]); rank 0 is the argmax,
        slots beyond M are (-inf, -1)."""
        lo, hi = self._constraint_bounds(lo, hi)
        lower = _f64(lower)
        upper = _f64(upper)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError("cell bounds must be two C x m arrays of one shape (C = 0: two empty (0, m) arrays)")
        C_, m = lower.shape
        mt = m + len(lo)
        best = np.empty(int(k))
        idx = np.empty(int(k), dtype=np.int64)
        vals = np.empty(self.M) if return_values else None
        pof = np.empty(self.M) if return_pof else None
        mu = np.empty((self.M, mt)) if return_moments else None
        mse = np.empty((self.M, mt)) if return_moments else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(self._lib.bogp_sweep_ehvi_constrained(self._h, int(m), int(C_), _ptr(lower) if C_ else None, _ptr(upper) if C_ else None,
                                                          len(lo), _ptr(lo), _ptr(hi), int(k), _ptr(best), idx.ctypes.data_as(_lp),
                                                          _ptr(vals), _ptr(pof), _ptr(mu), _ptr(mse)))  # fmt: skip
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_pof:
            out += (pof,)
        if return_moments:
            out += (mu, mse)
        return out

    # -- Kriging-believer batches (bogp_api_believer.hip): what the four families' methods do alike ----------------
    @staticmethod
    def _constraint_bounds(lo, hi):
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if len(lo) != len(hi):
            raise ValueError("lo and hi must hold one bound per constraint each")
        return lo, hi

    def _pending(self, pending):
        """(the pending rows (n, d) or None, n)"""
        pend = None if pending is None or len(pending) == 0 else _f64(pending)
        if pend is not None and (pend.ndim != 2 or pend.shape[1] != self.d):
            raise ValueError("pending points must have shape (n, %d)" % self.d)
        return pend, 0 if pend is None else pend.shape[0]

    @staticmethod
    def _front(front, m):
        """The observed front (n, m), or None for an empty one."""
        F = None if front is None or np.size(front) == 0 else _f64(front)
        if F is not None and (F.ndim != 2 or F.shape[1] != m):
            raise ValueError("the front must have shape (n, %d)" % m)
        return F

    def _believer_outputs(self, q, n_pend, m=None):
        """(the result dict every family starts from: q winners, their rows, their m means, n + q pivots; the pointers to those
        arrays in the order every entry takes them)"""
        q = max(q, 0)
        val, idx, x, piv = np.empty(q), np.empty(q, dtype=np.int64), np.empty((q, self.d)), np.empty(n_pend + q)
        if m is None:
            return dict(best_val=val, best_idx=idx, best_x=x, pivots=piv), (_ptr(val), idx.ctypes.data_as(_lp), _ptr(x), _ptr(piv))
        mu = np.empty((q, m))
        return (dict(best_val=val, best_idx=idx, best_x=x, best_mu=mu, pivots=piv),
                (_ptr(val), idx.ctypes.data_as(_lp), _ptr(x), _ptr(mu), _ptr(piv)))  # fmt: skip

    def _believer_call(self, fn, *args, unsupported=False):
        """One believer entry: no sweep's winners stay readable behind it; `unsupported`: what the library refuses as unsupported
        raises NotImplementedError with its message."""
        self._last_q, self._last_topk = -1, (-1, -1)
        try:
            self._check(fn(self._h, *args))
        except BogpError as e:
            if unsupported and e.code == ERR_UNSUPPORTED:
                raise NotImplementedError(str(e)) from None
            raise

    def _believer_last(self, fn, criterion_key):
        """The five figures of a multi-target family's *_last entry: producer, solves, k_believer, the criterion kernel, passes."""
        c, s, u, e, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int()
        self._check(fn(self._h, C.cast(C.byref(c), _dp), C.cast(C.byref(s), _dp), C.cast(C.byref(u), _dp), C.cast(C.byref(e), _dp),
                       C.cast(C.byref(n), _ip)))  # fmt: skip
        return {"corr_ms": c.value, "solve_ms": s.value, "update_ms": u.value, criterion_key: e.value, "n_passes": n.value}

    def sweep_believer(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize=True, pending=None, believe_plugin=True,
                       return_values=False):
        """Kriging-believer batch over the current candidates (bogp_sweep_believer): step j maximises criterion j on the mean and
        on the variance conditioned on the `pending` rows (n, d) and on the winners of the steps before it.  Returns a dict:
        best_val (q,), best_idx (q,), best_x (q, d), pivots (n + q,) and, with return_values, acq (q, M) and mse (q, M)."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        pend, n_pend = self._pending(pending)
        out, winners = self._believer_outputs(q, n_pend)
        vals = np.empty((q, self.M)) if return_values else None
        mse = np.empty((q, self.M)) if return_values else None
        self._believer_call(self._lib.bogp_sweep_believer, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                            int(bool(believe_plugin)), _ptr(pend), n_pend, *winners, _ptr(vals), _ptr(mse))  # fmt: skip
        if return_values:
            out.update(acq=vals, mse=mse)
        return out

    def believer_last(self) -> dict:
        """Producer, solve and k_believer time (ms) and the candidate passes of the last sweep_believer (bogp_believer_last)."""
        c, s, b, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        self._check(self._lib.bogp_believer_last(self._h, C.cast(C.byref(c), _dp), C.cast(C.byref(s), _dp), C.cast(C.byref(b), _dp),
                                                 C.cast(C.byref(n), _ip)))  # fmt: skip
        return dict(corr_ms=c.value, solve_ms=s.value, believer_ms=b.value, n_passes=n.value)

    def _thompson_draw(self, draw, ncol=None):
        """A draw's arrays as the entries take them: (L, omega, phase, weights, eps or None), checked against `ncol` columns -- the
        weights' own count (and so q) where it is None."""
        omega, phase, weights = _f64(draw.omega), _f64(draw.phase), _f64(draw.weights)
        eps = None if draw.eps is None else _f64(draw.eps)
        bad = weights.ndim != 2 or omega.ndim != 2 or omega.shape != (len(phase), self.d) or weights.shape[0] != len(phase)
        if bad or (ncol is not None and weights.shape[1] != ncol):
            raise ValueError("a draw holds omega (L, %d), phase (L,) and weights (L, %s)" % (self.d, "q" if ncol is None else ncol))
        if eps is not None and eps.shape != (self.N, weights.shape[1]):
            raise ValueError("eps must have shape (%d, %d)" % (self.N, weights.shape[1]))
        return len(phase), omega, phase, weights, eps

    def _thompson_call(self, fn, *args):
        """One Thompson entry: no sweep's winners stay readable behind it; what the library refuses as unsupported raises
        NotImplementedError with its message."""
        self._believer_call(fn, *args, unsupported=True)

    def _thompson_last(self, fn):
        """The four figures of a family's *_last entry: producer, draw at the training rows with its solves, the kernel, chunks."""
        c, s, p, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        self._check(fn(self._h, C.cast(C.byref(c), _dp), C.cast(C.byref(s), _dp), C.cast(C.byref(p), _dp), C.cast(C.byref(n), _ip)))
        return dict(corr_ms=c.value, solve_ms=s.value, paths_ms=p.value, n_chunks=n.value)

    def sweep_thompson(self, draw, minimize=True, k: int = 1, conditioned=True, return_values=False):
        """q sample paths of the committed model over the current candidates (bogp_sweep_thompson), each with its k best rows.
        `draw`: the arrays of `bogp.thompson.draw` -- omega (L, d), phase (L,), weights (L, q), eps (N, q) or None.  Returns a dict:
        best_val (q, k) in the criterion's sign (-path when minimising), best_idx (q, k), best_x (q, k, d) -- rank 0 is the argmax,
        slots beyond M are (-inf, -1) -- coef = (gt (N, q), bt (q,)) and, with return_values, paths (q, M).  What the library
        refuses as unsupported (a mode, kernel, trend, ...) raises NotImplementedError with its message."""
        L, omega, phase, weights, eps = self._thompson_draw(draw)
        q, k = weights.shape[1], int(k)
        best = np.empty((q, k))
        idx = np.empty((q, k), dtype=np.int64)
        bx = np.empty((q, k, self.d))
        paths = np.empty((q, self.M)) if return_values else None
        coef = np.empty((self.N + 1, q))
        self._thompson_call(self._lib.bogp_sweep_thompson, q, L, _ptr(omega), _ptr(phase), _ptr(weights), _ptr(eps), int(bool(conditioned)),
                            int(bool(minimize)), k, _ptr(best), idx.ctypes.data_as(_lp), _ptr(bx), _ptr(paths), _ptr(coef))  # fmt: skip
        out = dict(best_val=best, best_idx=idx, best_x=bx, coef=(coef[:-1].copy(), coef[-1].copy()))
        if return_values:
            out["paths"] = paths
        return out

    def thompson_last(self) -> dict:
        """Producer time, time of the draw at the training rows with its solves, k_thompson time over the candidates (ms) and the
        chunks of the last sweep_thompson (bogp_thompson_last)."""
        return self._thompson_last(self._lib.bogp_thompson_last)

    def sweep_thompson_constrained(self, draw, q: int, lo, hi, minimize=True, k: int = 1, return_values=False):
        """Joint sample paths of the objective and the modelled constraints of the committed multi-target model over the current
        candidates (bogp_sweep_thompson_constrained): `q` batch members of m = 1 + len(lo) targets, q m <= 16 columns.  `draw`: the
        arrays of `bogp.thompson.draw_multi` -- omega (L, d), phase (L,), weights (L, q m), eps (N, q m) or None, column j m + t.
        Returns a dict: best_val / best_idx (q, 2, k) -- per member the k best rows of A (the objective path, negated when
        minimising, where the drawn constraints hold, else -inf), then of B (minus the largest scaled excess) -- best_x
        (q, 2, k, d), coef (N, q m) and, with return_values, paths (q, m, M) in the paths' own sign.  What the library refuses as
        unsupported raises NotImplementedError with its message."""
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        q, k, m = int(q), int(k), len(lo) + 1
        if len(hi) != len(lo):
            raise ValueError("lo and hi hold one bound per constraint")
        L, omega, phase, weights, eps = self._thompson_draw(draw, q * m)
        qa, ka = max(q, 1), max(k, 1)
        best = np.empty((qa, 2, ka))
        idx = np.empty((qa, 2, ka), dtype=np.int64)
        bx = np.empty((qa, 2, ka, self.d))
        paths = np.empty((qa, m, self.M)) if return_values else None
        coef = np.empty((self.N, qa * m))
        self._thompson_call(self._lib.bogp_sweep_thompson_constrained, q, L, _ptr(omega), _ptr(phase), _ptr(weights), _ptr(eps),
                            int(bool(minimize)), len(lo), _ptr(lo), _ptr(hi), k, _ptr(best), idx.ctypes.data_as(_lp), _ptr(bx), _ptr(paths),
                            _ptr(coef))  # fmt: skip
        out = dict(best_val=best, best_idx=idx, best_x=bx, coef=coef)
        if return_values:
            out["paths"] = paths
        return out

    def thompson_constrained_last(self) -> dict:
        """Producer time, time of the draw at the training rows with its solves, k_thompson_constrained time over the candidates
        (ms) and the chunks of the last sweep_thompson_constrained (bogp_thompson_constrained_last)."""
        return self._thompson_last(self._lib.bogp_thompson_constrained_last)

    def sweep_believer_ehvi(self, front, ref_point, q: int, pending=None, believe_front=True, return_values=False):
        """Kriging-believer batch under EHVI over the current candidates (bogp_sweep_believer_ehvi): step j maximises EHVI on the m
        means and on the variances conditioned on the `pending` rows (n, d) and on the winners of the steps before it, over the cells
        of the front of `front` (n_front, m; may be empty) above `ref_point` -- extended by every believed mean when `believe_front`.
        Returns a dict: best_val (q,), best_idx (q,), best_x (q, d), best_mu (q, m), pivots (n + q,), n_cells (q,) and, with
        return_values, ehvi (q, M) and mse (q, M, m)."""
        r = _f64(ref_point).ravel()
        m, q = len(r), int(q)
        F = self._front(front, m)
        pend, n_pend = self._pending(pending)
        qa = max(q, 0)
        out, winners = self._believer_outputs(q, n_pend, m)
        nc = out["n_cells"] = np.zeros(qa, dtype=np.int32)
        vals = np.empty((qa, self.M)) if return_values else None
        mse = np.empty((qa, self.M, m)) if return_values else None
        self._believer_call(self._lib.bogp_sweep_believer_ehvi, m, q, _ptr(r), _ptr(F), 0 if F is None else len(F), int(bool(believe_front)),
                            _ptr(pend), n_pend, *winners, nc.ctypes.data_as(_ip), _ptr(vals), _ptr(mse))  # fmt: skip
        if return_values:
            out.update(ehvi=vals, mse=mse)
        return out

    def believer_ehvi_last(self) -> dict:
        """Producer, solve, k_believer and k_believer_ehvi time (ms) and the candidate passes of the last sweep_believer_ehvi
        (bogp_believer_ehvi_last)."""
        return self._believer_last(self._lib.bogp_believer_ehvi_last, "ehvi_ms")

    def sweep_believer_constrained(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize, lo, hi, pending=None, believe_plugin=True,
                                   return_values=False):
        """Kriging-believer batch under modelled constraints over the current candidates (bogp_sweep_believer_constrained): step j
        maximises criterion j of `acq` (EI, EpsilonPI, MGFI on target 0; ACQ_NONE: 1) x the constraints' probabilities of feasibility
        in [lo, hi], on the m means and on the variances conditioned on the `pending` rows (n, d) and on the winners of the steps
        before it.  With `believe_plugin` a believed point whose means are feasible lowers the plugin.  Returns a dict: best_val (q,),
        best_idx (q,), best_x (q, d), best_mu (q, m), pivots (n + q,), plugins (q,) and, with return_values, acq (q, M), pof (q, M)
        and mse (q, M, m).  What the library refuses as unsupported (a forest, a lift, a polynomial basis, several ranks) raises
        NotImplementedError with its message."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        lo, hi = self._constraint_bounds(lo, hi)
        m = len(lo) + 1
        pend, n_pend = self._pending(pending)
        out, winners = self._believer_outputs(q, n_pend, m)
        plugs = out["plugins"] = np.empty(q)
        vals = np.empty((q, self.M)) if return_values else None
        pof = np.empty((q, self.M)) if return_values else None
        mse = np.empty((q, self.M, m)) if return_values else None
        self._believer_call(self._lib.bogp_sweep_believer_constrained, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin),
                            int(bool(minimize)), int(bool(believe_plugin)), len(lo), _ptr(lo), _ptr(hi), _ptr(pend), n_pend, *winners,
                            _ptr(plugs), _ptr(vals), _ptr(pof), _ptr(mse), unsupported=True)  # fmt: skip
        if return_values:
            out.update(acq=vals, pof=pof, mse=mse)
        return out

    def believer_constrained_last(self) -> dict:
        """Producer, solve, k_believer and k_believer_constrained time (ms) and the candidate passes of the last
        sweep_believer_constrained (bogp_believer_constrained_last)."""
        return self._believer_last(self._lib.bogp_believer_constrained_last, "criterion_ms")

    def sweep_believer_ehvi_constrained(self, front, ref_point, q: int, lo, hi, pending=None, believe_front=True, feasibility_only=False,
                                        return_values=False):
        """Kriging-believer batch under constrained EHVI over the current candidates (bogp_sweep_believer_ehvi_constrained): step j
        maximises EHVI of the first m = len(ref_point) targets x the probabilities that the remaining c = len(lo) targets are feasible
        in [lo, hi], on the m + c means and on the variances conditioned on the `pending` rows (n, d) and on the winners of the steps
        before it, over the cells of the front of `front` (the objective rows of the feasible observations, (n_front, m); may be
        empty) above `ref_point`.  With `believe_front` the objective part of a believed mean joins that front when every constraint
        mean lies in its closed interval.  `feasibility_only`: no feasible observation exists; every step maximises the probability of
        feasibility alone (no cells, `front` must be empty).  Returns a dict: best_val (q,), best_idx (q,), best_x (q, d), best_mu
        (q, m + c), pivots (n + q,), n_cells (q,) and, with return_values, val (q, M), pof (q, M) and mse (q, M, m + c).  What the
        library refuses as unsupported (a forest, a lift, a polynomial basis, several ranks) raises NotImplementedError with its
        message."""
        r = _f64(ref_point).ravel()
        m, q = len(r), int(q)
        lo, hi = self._constraint_bounds(lo, hi)
        mt = m + len(lo)
        F = self._front(front, m)
        pend, n_pend = self._pending(pending)
        qa = max(q, 0)
        out, winners = self._believer_outputs(q, n_pend, mt)
        nc = out["n_cells"] = np.zeros(qa, dtype=np.int32)
        vals = np.empty((qa, self.M)) if return_values else None
        pof = np.empty((qa, self.M)) if return_values else None
        mse = np.empty((qa, self.M, mt)) if return_values else None
        self._believer_call(self._lib.bogp_sweep_believer_ehvi_constrained, m, q, _ptr(r), _ptr(F), 0 if F is None else len(F),
                            int(bool(feasibility_only)), int(bool(believe_front)), len(lo), _ptr(lo), _ptr(hi), _ptr(pend), n_pend,
                            *winners, nc.ctypes.data_as(_ip), _ptr(vals), _ptr(pof), _ptr(mse), unsupported=True)  # fmt: skip
        if return_values:
            out.update(val=vals, pof=pof, mse=mse)
        return out

    def believer_ehvi_constrained_last(self) -> dict:
        """Producer, solve, k_believer and k_believer_ehvi_constrained time (ms) and the candidate passes of the last
        sweep_believer_ehvi_constrained (bogp_believer_ehvi_constrained_last)."""
        return self._believer_last(self._lib.bogp_believer_ehvi_constrained_last, "criterion_ms")

    # -- lift of a reduced search space (PCA-BO; bogp_api_lift.hip) ------------------------------------------------
    def set_lift(self, A, mean, center, lo, hi):
        """The lift of the lifted sweeps that follow (bogp_lift_set): A (r, D) = pca.components_ with r = the model's d, mean (D),
        center (D, or None = 0), lo / hi (D) the original box.  Stays on the engine until clear_lift()."""
        A = _f64(A)
        if A.ndim != 2 or A.shape[0] != self.d:
            raise ValueError("A must have shape (%d, D)" % self.d)
        D = A.shape[1]
        mean, lo, hi = _f64(mean).ravel(), _f64(lo).ravel(), _f64(hi).ravel()
        center = None if center is None else _f64(center).ravel()
        if any(v is not None and len(v) != D for v in (mean, center, lo, hi)):
            raise ValueError("mean, center, lo and hi must have D = %d entries" % D)
        self._check(self._lib.bogp_lift_set(self._h, int(D), _ptr(A), _ptr(mean), _ptr(center), _ptr(lo), _ptr(hi)))

    def clear_lift(self):
        self._check(self._lib.bogp_lift_clear(self._h))

    def lift_sweep_topk(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize=True, k: int = 1, return_values=False,
                        return_penalty=False):
        """k best candidates per criterion under the engine's lift (bogp_lift_sweep_topk): a row whose lifted point leaves the box
        competes with its penalty, a feasible row with its criterion value.  (values (q, k), indices (q, k), n_feasible
        [, values (q, M)][, penalty (M,)])."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        best = np.empty((q, int(k)))
        idx = np.empty((q, int(k)), dtype=np.int64)
        nf = C.c_int64()
        vals = np.empty((q, self.M)) if return_values else None
        pen = np.empty(self.M) if return_penalty else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(self._lib.bogp_lift_sweep_topk(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                                   int(k), _ptr(best), idx.ctypes.data_as(_lp), C.cast(C.byref(nf), _lp), _ptr(vals),
                                                   _ptr(pen)))  # fmt: skip
        out = (best, idx, int(nf.value))
        if return_values:
            out += (vals,)
        if return_penalty:
            out += (pen,)
        return out

    def lift_last(self) -> dict:
        """Feasible rows, filter time and merge + ranking time (ms) of the last lifted sweep (bogp_lift_last)."""
        nf, f, m = C.c_int64(), C.c_double(), C.c_double()
        self._check(self._lib.bogp_lift_last(self._h, C.cast(C.byref(nf), _lp), C.cast(C.byref(f), _dp), C.cast(C.byref(m), _dp)))
        return {"n_feasible": int(nf.value), "filter_ms": f.value, "merge_ms": m.value}

    # -- packed regression forest (the second model kind; bogp_api_forest.hip) ----------------------------------
    def forest_set(self, d: int, tree_offset, feature, threshold, left, right, value, test=None):
        """T trees over d columns as flat arrays (scikit-learn's layout per tree; `forest.pack` builds them).  Establishes d for
        the candidate calls.  Raises on a malformed forest: validation is host-side, nothing is launched."""
        off = np.ascontiguousarray(tree_offset, dtype=np.int64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        feature, left, right = i32(feature), i32(left), i32(right)
        threshold, value = _f64(threshold).ravel(), _f64(value).ravel()
        n = int(off[-1]) if len(off) else 0
        if not (len(feature) == len(left) == len(right) == len(threshold) == len(value) == n):
            raise ValueError("the node arrays must all have tree_offset[-1] = %d entries" % n)
        tst = None if test is None else i32(test)
        if tst is not None and len(tst) != n:
            raise ValueError("test must have %d entries" % n)
        self._check(self._lib.bogp_forest_set(self._h, len(off) - 1, int(d), off.ctypes.data_as(_lp), feature.ctypes.data_as(_ip),
                                              _ptr(threshold), left.ctypes.data_as(_ip), right.ctypes.data_as(_ip), _ptr(value),
                                              None if tst is None else tst.ctypes.data_as(_ip)))  # fmt: skip
        if int(d) != self.d:
            self.M = 0
        self.d, self.N, self.forest_T = int(d), 0, len(off) - 1
        self._last_q, self._last_topk = -1, (-1, -1)

    def forest_info(self) -> dict:
        out = np.zeros(7, dtype=np.int64)
        self._check(self._lib.bogp_forest_info(self._h, out.ctypes.data_as(_lp)))
        return dict(zip(("T", "d", "nodes", "leaves", "depth", "bytes", "lds_bytes"), (int(v) for v in out)))

    def forest_predict(self, eval_MSE=True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        mu = np.empty(self.M)
        mse = np.empty(self.M) if eval_MSE else None
        self._check(self._lib.bogp_forest_predict(self._h, _ptr(mu), _ptr(mse)))
        return mu, mse

    def forest_leaves(self, first_row: int, n: int) -> np.ndarray:
        """Per-tree predictions (n, T) of candidate rows [first_row, first_row + n)."""
        out = np.empty((int(n), int(getattr(self, "forest_T", 0))))
        self._check(self._lib.bogp_forest_leaves(self._h, int(first_row), int(n), _ptr(out)))
        return out

    def forest_sweep_topk(self, acq: Sequence[Tuple[int, float]], plugin: float, minimize=True, k: int = 1, return_values=False):
        """q criteria of the forest's moments over the current candidates: (values (q, k), indices (q, k)[, acq (q, M)])."""
        q = len(acq)
        ids, pars = _pack_acq(acq)
        best = np.empty((q, int(k)))
        idx = np.empty((q, int(k)), dtype=np.int64)
        vals = np.empty((q, self.M)) if return_values else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(
            self._lib.bogp_forest_sweep_topk(self._h, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin), int(bool(minimize)),
                                             int(k), _ptr(best), idx.ctypes.data_as(_lp), _ptr(vals))
        )  # fmt: skip
        self._last_q = q
        if int(k) > 1:
            self._last_topk = (q, int(k))
        return (best, idx, vals) if return_values else (best, idx)

    # -- forests with several outputs (k_forest_ehvi) --------------------------------------------------------------
    def forest_set_multi(self, d: int, m: int, tree_offset, feature, threshold, left, right, value, test=None):
        """`forest_set` for a forest whose leaves hold m >= 2 values: `value` is (nodes, m) (scikit-learn's `tree_.value[:, :, 0]`)."""
        off = np.ascontiguousarray(tree_offset, dtype=np.int64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        feature, left, right = i32(feature), i32(left), i32(right)
        threshold, value = _f64(threshold).ravel(), _f64(value)
        n = int(off[-1]) if len(off) else 0
        if not (len(feature) == len(left) == len(right) == len(threshold) == n) or value.shape != (n, int(m)):
            raise ValueError("the node arrays must have tree_offset[-1] = %d entries and value the shape (%d, %d)" % (n, n, int(m)))
        tst = None if test is None else i32(test)
        if tst is not None and len(tst) != n:
            raise ValueError("test must have %d entries" % n)
        self._check(self._lib.bogp_forest_set_multi(self._h, len(off) - 1, int(d), int(m), off.ctypes.data_as(_lp),
                                                    feature.ctypes.data_as(_ip), _ptr(threshold), left.ctypes.data_as(_ip),
                                                    right.ctypes.data_as(_ip), _ptr(value),
                                                    None if tst is None else tst.ctypes.data_as(_ip)))  # fmt: skip
        if int(d) != self.d:
            self.M = 0
        self.d, self.N, self.forest_T = int(d), 0, len(off) - 1
        self._last_q, self._last_topk = -1, (-1, -1)

    def forest_outputs(self) -> int:
        """Outputs a leaf of the engine's forest holds (0 without a forest)."""
        return int(self._lib.bogp_forest_outputs(self._h))

    def forest_predict_multi(self, eval_MSE=True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """mu (M, m) and MSE (M, m) of a forest with several outputs over the current candidates."""
        m = self.forest_outputs()
        mu = np.empty((self.M, m))
        mse = np.empty((self.M, m)) if eval_MSE else None
        self._check(self._lib.bogp_forest_predict_multi(self._h, _ptr(mu), _ptr(mse)))
        return mu, mse

    def forest_leaves_multi(self, first_row: int, n: int) -> np.ndarray:
        """Per-tree, per-output predictions (n, T, m) of candidate rows [first_row, first_row + n)."""
        out = np.empty((int(n), int(getattr(self, "forest_T", 0)), self.forest_outputs()))
        self._check(self._lib.bogp_forest_leaves_multi(self._h, int(first_row), int(n), _ptr(out)))
        return out

    def forest_sweep_ehvi(self, lower, upper, k: int = 1, return_values=False, return_moments=False):
        """Expected hypervolume improvement on the moments of a forest with several outputs, over the current candidates:
        arguments and results as `sweep_ehvi` (bogp_forest_sweep_ehvi)."""
        lower = _f64(lower)
        upper = _f64(upper)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError("cell bounds must be two C x m arrays of one shape")
        C_, m = lower.shape
        best = np.empty(int(k))
        idx = np.empty(int(k), dtype=np.int64)
        vals = np.empty(self.M) if return_values else None
        mu = np.empty((self.M, m)) if return_moments else None
        mse = np.empty((self.M, m)) if return_moments else None
        self._last_q, self._last_topk = -1, (-1, -1)
        self._check(self._lib.bogp_forest_sweep_ehvi(self._h, int(m), int(C_), _ptr(lower), _ptr(upper), int(k), _ptr(best),
                                                     idx.ctypes.data_as(_lp), _ptr(vals), _ptr(mu), _ptr(mse)))  # fmt: skip
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out

    def generate_candidates_mixed(self, kind, lo, hi, n_levels, M: int, seed: int = 0, first_row: int = 0):
        """M rows of a mixed space drawn ON the device: column k is real (kind 0: lo + (hi - lo) u, then the candidate transform)
        or discrete (kind 1: index = min(floor(u L), L - 1), value lo + index (hi - lo) / (L - 1)) -- bogp_candidates_generate_mixed."""
        kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
        nl = np.ascontiguousarray(n_levels, dtype=np.int32).ravel()
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if not (len(kind) == len(nl) == len(lo) == len(hi) == self.d):
            raise ValueError("kind, lo, hi and n_levels must have %d entries" % self.d)
        self._check(self._lib.bogp_candidates_generate_mixed(self._h, kind.ctypes.data_as(_ip), _ptr(lo), _ptr(hi), nl.ctypes.data_as(_ip),
                                                             int(M), C.c_uint64(int(seed) & (2**64 - 1)), int(first_row)))  # fmt: skip
        self.M = int(M)
        self._last_q, self._last_topk = -1, (-1, -1)
        self._keep = None

    def gradient(self, x):
        x = _f64(x).ravel()
        if len(x) != self.d:
            raise Exception("x does not have the right size!")
        dmu, dmse = np.empty(self.d), np.empty(self.d)
        self._check(self._lib.bogp_gradient(self._h, _ptr(x), _ptr(dmu), _ptr(dmse)))
        return dmu, dmse

    def point_eval(self, x, acq: Sequence[Tuple[int, float]] = (), plugin: float = 0.0, minimize: bool = True):
        """mu, mse, dmu (d,), dmse (d,), criterion values (q,) at ONE point with one device round trip
        (bogp_point_eval: what `criterion(x, return_dx=True)` needs).  Constant trend basis.
        This is the call the reference's L-BFGS-B loop makes thousands of times per ask(): the ctypes argument objects are
        built once per (d, criteria) and re-used, so that the host side of a call is a few microseconds."""
        key = (self.d, tuple(acq))
        c = self.__dict__.get("_pe_cache")
        if c is None or c[0] != key:
            q = len(acq)
            ids = np.ascontiguousarray([a for a, _ in acq], dtype=np.int32)
            pars = np.ascontiguousarray([p for _, p in acq], dtype=np.float64)
            xb, out = np.empty(self.d), np.empty(2 + 2 * self.d + max(q, 1))
            po = out.ctypes.data
            c = (key, q, xb, out, ids, pars, _ptr(xb), ids.ctypes.data_as(_ip) if q else None, _ptr(pars) if q else None,
                 C.cast(po, _dp), C.cast(po + 8, _dp), C.cast(po + 16, _dp), C.cast(po + 16 + 8 * self.d, _dp),
                 C.cast(po + 16 + 16 * self.d, _dp) if q else None)  # fmt: skip
            self._pe_cache = c
        _, q, xb, out, _, _, px, pids, ppars, pmu, pmse, pdmu, pdmse, pvals = c
        x = np.asarray(x, dtype=np.float64)
        if x.size != self.d:
            raise Exception("x does not have the right size!")
        xb[:] = x.ravel()
        rc = self._lib.bogp_point_eval(self._h, px, q, pids, ppars, float(plugin), 1 if minimize else 0, pmu, pmse, pdmu, pdmse, pvals)
        if rc:
            self._check(rc)
        d = self.d
        return float(out[0]), float(out[1]), out[2 : 2 + d].copy(), out[2 + d : 2 + 2 * d].copy(), out[2 + 2 * d : 2 + 2 * d + q].copy()

    def point_eval_batch(self, Xb, acq: Sequence[Tuple[int, float]] = (), plugin: float = 0.0, minimize: bool = True,
                         return_dx: bool = True):
        """(mu (B,), mse (B,), dmu (B, d), dmse (B, d), values (B, q), dvalues (B, q, d) or None) at the B rows of `Xb` in ONE
        device round trip (bogp_point_eval_batch): the criteria's input-gradients are the reference's `return_dx` chain rule
        evaluated on the device.  Constant trend basis."""
        Xb = _f64(Xb)
        if Xb.ndim != 2 or Xb.shape[1] != self.d:
            raise Exception("x does not have the right size!")
        B, q = Xb.shape[0], len(acq)
        ids = np.ascontiguousarray([a for a, _ in acq], dtype=np.int32)
        pars = np.ascontiguousarray([p for _, p in acq], dtype=np.float64)
        mu, mse = np.empty(B), np.empty(B)
        dmu, dmse = np.empty((B, self.d)), np.empty((B, self.d))
        vals = np.empty((B, max(q, 1)))
        dvals = np.empty((B, max(q, 1), self.d)) if (return_dx and q) else None
        self._check(
            self._lib.bogp_point_eval_batch(self._h, _ptr(Xb), B, q, ids.ctypes.data_as(_ip) if q else None, _ptr(pars) if q else None,
                                            float(plugin), int(bool(minimize)), _ptr(mu), _ptr(mse), _ptr(dmu), _ptr(dmse),
                                            _ptr(vals) if q else None, _ptr(dvals))
        )  # fmt: skip
        return mu, mse, dmu, dmse, vals[:, :q], (dvals[:, :q] if dvals is not None else None)

    def _rows(self, X):
        """The points of a multi-target call as B x d: one point may come as a vector."""
        X = np.atleast_2d(_f64(X))
        if X.ndim != 2 or X.shape[1] != self.d:
            raise Exception("x does not have the right size!")
        return X

    def _polish_io(self, X0, lo, hi, names):
        """The starts (B x d) and the box of a polish checked, its outputs allocated: (X0, lo, hi, B, Xo, fo, ne)."""
        if X0.ndim != 2 or X0.shape[1] != self.d:
            raise Exception("x does not have the right size!")
        lo, hi = _f64(lo).ravel(), _f64(hi).ravel()
        if len(lo) != self.d or len(hi) != self.d:
            raise ValueError(names + " must have d entries")
        B = X0.shape[0]
        return X0, lo, hi, B, np.empty((B, self.d)), np.empty(B), np.zeros(B, dtype=np.int32)

    def polish(self, X0, lo, hi, acq: Tuple[int, float], plugin: float = 0.0, minimize: bool = True, max_evals: int = 50,
               pgtol: float = 1e-8, factr: float = 1e6):
        """Lock-step multi-start local maximisation of one criterion inside the box (bogp_polish): (points (B, d), values (B,),
        evaluations used (B,)); values[i] >= the criterion at X0[i]."""
        X0, lo, hi, B, Xo, fo, ne = self._polish_io(_f64(X0), lo, hi, "lo / hi")
        self._check(
            self._lib.bogp_polish(self._h, _ptr(X0), B, _ptr(lo), _ptr(hi), int(acq[0]), float(acq[1]), float(plugin),
                                  int(bool(minimize)), int(max_evals), float(pgtol), float(factr), _ptr(Xo), _ptr(fo),
                                  ne.ctypes.data_as(_ip))
        )  # fmt: skip
        return Xo, fo, ne

    @staticmethod
    def _cells(lower, upper):
        lower, upper = _f64(lower), _f64(upper)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError("cell bounds must be two C x m arrays of one shape")
        return lower, upper

    def point_eval_ehvi(self, X, lower, upper, moments: bool = False):
        """EHVI of the committed multi-target model and its input gradient at the rows of `X` (B x d) in ONE device round trip
        (bogp_point_eval_ehvi), for the cells (lower, upper) (C x m each; upper may hold +inf): (ehvi (B,), dehvi (B, d)) and,
        with `moments`, also mu (B, m), mse (B, m), dmu (B, m, d), dmse (B, m, d).  Cells equal to those of the call before are
        not uploaded again."""
        X = self._rows(X)
        lower, upper = self._cells(lower, upper)
        C_, m = lower.shape
        B, d = X.shape[0], self.d
        ehvi, dehvi = np.empty(B), np.empty((B, d))
        mom = (np.empty((B, m)), np.empty((B, m)), np.empty((B, m, d)), np.empty((B, m, d))) if moments else (None,) * 4
        rc = self._lib.bogp_point_eval_ehvi(self._h, _ptr(X), B, int(m), int(C_), _ptr(lower), _ptr(upper), _ptr(ehvi), _ptr(dehvi),
                                            *(_ptr(a) for a in mom))  # fmt: skip
        if rc:
            self._check(rc)
        return (ehvi, dehvi) + (mom if moments else ())

    def polish_ehvi(self, starts, lo, hi, lower, upper, max_evals: int = 50, pgtol: float = 1e-8, factr: float = 1e6):
        """Lock-step multi-start local maximisation of EHVI inside the box (bogp_polish_ehvi): (points (B, d), values (B,),
        evaluations used (B,)); values[i] >= EHVI at starts[i] clipped into the box."""
        X0, lo, hi, B, Xo, fo, ne = self._polish_io(self._rows(starts), lo, hi, "lo / hi")
        lower, upper = self._cells(lower, upper)
        C_, m = lower.shape
        self._check(
            self._lib.bogp_polish_ehvi(self._h, _ptr(X0), B, _ptr(lo), _ptr(hi), int(m), int(C_), _ptr(lower), _ptr(upper),
                                       int(max_evals), float(pgtol), float(factr), _ptr(Xo), _ptr(fo), ne.ctypes.data_as(_ip))
        )  # fmt: skip
        return Xo, fo, ne

    def point_eval_constrained(self, X, acq: Sequence[Tuple[int, float]], plugin: float, minimize, lo, hi, moments: bool = False):
        """q feasibility-weighted criteria of the committed multi-target model and their input gradients at the rows of `X` (B x d) in
        ONE device round trip (bogp_point_eval_constrained); criteria, plugin, direction and the constraints' bounds as
        `sweep_constrained`: (acq (B, q), dacq (B, q, d)) and, with `moments`, also pof (B,), dpof (B, d), mu (B, m), mse (B, m),
        dmu (B, m, d), dmse (B, m, d)."""
        X = self._rows(X)
        lo, hi = self._constraint_bounds(lo, hi)
        q, m = len(acq), len(lo) + 1
        ids, pars = _pack_acq(acq)
        B, d = X.shape[0], self.d
        vals, dvals = np.empty((B, q)), np.empty((B, q, d))
        mom = ((np.empty(B), np.empty((B, d)), np.empty((B, m)), np.empty((B, m)), np.empty((B, m, d)), np.empty((B, m, d)))
               if moments else (None,) * 6)  # fmt: skip
        rc = self._lib.bogp_point_eval_constrained(self._h, _ptr(X), B, q, ids.ctypes.data_as(_ip), _ptr(pars), float(plugin),
                                                   int(bool(minimize)), len(lo), _ptr(lo), _ptr(hi), _ptr(vals), _ptr(dvals),
                                                   *(_ptr(a) for a in mom))  # fmt: skip
        if rc:
            self._check(rc)
        return (vals, dvals) + (mom if moments else ())

    def polish_constrained(self, starts, box_lo, box_hi, acq: Tuple[int, float], plugin: float, minimize, lo, hi, max_evals: int = 50,
                           pgtol: float = 1e-8, factr: float = 1e6):
        """Lock-step multi-start local maximisation of one feasibility-weighted criterion inside the box (bogp_polish_constrained):
        (points (B, d), values (B,), evaluations used (B,)); values[i] >= the criterion at starts[i] clipped into the box."""
        X0, box_lo, box_hi, B, Xo, fo, ne = self._polish_io(self._rows(starts), box_lo, box_hi, "box_lo / box_hi")
        lo, hi = self._constraint_bounds(lo, hi)
        self._check(
            self._lib.bogp_polish_constrained(self._h, _ptr(X0), B, _ptr(box_lo), _ptr(box_hi), int(acq[0]),
                                              float(acq[1]) if acq[1] is not None else 0.0, float(plugin), int(bool(minimize)), len(lo),
                                              _ptr(lo), _ptr(hi), int(max_evals), float(pgtol), float(factr), _ptr(Xo), _ptr(fo),
                                              ne.ctypes.data_as(_ip))
        )  # fmt: skip
        return Xo, fo, ne

    def _constrained_cells(self, lower, upper, lo, hi):
        """The cells (C x m, C = 0: two empty (0, m) arrays) and the constraints' bounds of a constrained-EHVI point call, checked."""
        lo, hi = self._constraint_bounds(lo, hi)
        lower, upper = _f64(lower), _f64(upper)
        if lower.ndim != 2 or lower.shape != upper.shape:
            raise ValueError("cell bounds must be two C x m arrays of one shape (C = 0: two empty (0, m) arrays)")
        return lower, upper, lo, hi

    def point_eval_ehvi_constrained(self, X, lower, upper, lo, hi, moments: bool = False):
        """Feasibility-weighted EHVI of the committed multi-target model and its input gradient at the rows of `X` (B x d) in ONE device
        round trip (bogp_point_eval_ehvi_constrained); cells and constraint bounds as `sweep_ehvi_constrained`: (val (B,), dval (B, d))
        and, with `moments`, also pof (B,), dpof (B, d), ehvi (B,), dehvi (B, d), mu (B, m + c), mse (B, m + c), dmu (B, m + c, d),
        dmse (B, m + c, d).  Cells equal to those of the call before are not uploaded again."""
        X = self._rows(X)
        lower, upper, lo, hi = self._constrained_cells(lower, upper, lo, hi)
        C_, m = lower.shape
        mt = m + len(lo)
        B, d = X.shape[0], self.d
        val, dval = np.empty(B), np.empty((B, d))
        mom = ((np.empty(B), np.empty((B, d)), np.empty(B), np.empty((B, d)), np.empty((B, mt)), np.empty((B, mt)), np.empty((B, mt, d)),
                np.empty((B, mt, d))) if moments else (None,) * 8)  # fmt: skip
        rc = self._lib.bogp_point_eval_ehvi_constrained(self._h, _ptr(X), B, int(m), int(C_), _ptr(lower) if C_ else None,
                                                        _ptr(upper) if C_ else None, len(lo), _ptr(lo), _ptr(hi), _ptr(val), _ptr(dval),
                                                        *(_ptr(a) for a in mom))  # fmt: skip
        if rc:
            self._check(rc)
        return (val, dval) + (mom if moments else ())

    def polish_ehvi_constrained(self, starts, box_lo, box_hi, lower, upper, lo, hi, max_evals: int = 50, pgtol: float = 1e-8,
                                factr: float = 1e6):
        """Lock-step multi-start local maximisation of feasibility-weighted EHVI inside the box (bogp_polish_ehvi_constrained):
        (points (B, d), values (B,), evaluations used (B,)); values[i] >= the criterion at starts[i] clipped into the box."""
        X0, box_lo, box_hi, B, Xo, fo, ne = self._polish_io(self._rows(starts), box_lo, box_hi, "box_lo / box_hi")
        lower, upper, lo, hi = self._constrained_cells(lower, upper, lo, hi)
        C_, m = lower.shape
        self._check(
            self._lib.bogp_polish_ehvi_constrained(self._h, _ptr(X0), B, _ptr(box_lo), _ptr(box_hi), int(m), int(C_),
                                                   _ptr(lower) if C_ else None, _ptr(upper) if C_ else None, len(lo), _ptr(lo), _ptr(hi),
                                                   int(max_evals), float(pgtol), float(factr), _ptr(Xo), _ptr(fo), ne.ctypes.data_as(_ip))
        )  # fmt: skip
        return Xo, fo, ne

    feasibility_grad = staticmethod(feasibility_grad)

    def selftest_feasibility_grad(self, mu, mse, sigma2, lo, hi):
        """feasibility_grad of csrc/bogp_device.h on the device, one row of (mu, mse, sigma2, lo, hi) each (scalars or arrays, broadcast):
        (n, 3) = F, dF/dmu, dF/dsd (bogp_selftest_feasibility_grad)."""
        cols = np.broadcast_arrays(*[np.asarray(c, dtype=np.float64).ravel() for c in (mu, mse, sigma2, lo, hi)])
        rows = np.ascontiguousarray(np.stack(cols, axis=1))
        out = np.empty((len(rows), 3))
        self._check(self._lib.bogp_selftest_feasibility_grad(self._h, _ptr(rows), len(rows), _ptr(out)))
        return out

    def hessian(self, x) -> np.ndarray:
        """(d, d) Hessian of the posterior mean at x (squared exponential; constant / linear trend)."""
        x = _f64(x).ravel()
        if len(x) != self.d:
            raise Exception("x does not have the right size!")
        H = np.empty((self.d, self.d))
        self._check(self._lib.bogp_hessian(self._h, _ptr(x), _ptr(H)))
        return H

    def prior_corr(self, X1) -> np.ndarray:
        """(n1, n1) correlation matrix of the rows of X1 at the committed theta."""
        X1 = _f64(X1)
        if X1.ndim != 2 or X1.shape[1] != self.d:
            raise ValueError("X1 must have shape (n1, %d)" % self.d)
        R = np.empty((X1.shape[0], X1.shape[0]))
        self._check(self._lib.bogp_prior_corr(self._h, _ptr(X1), X1.shape[0], _ptr(R)))
        return R

    def gradient_batch(self, Xb):
        """(d mu / dx, d MSE / dx) at B points: two (B, d) arrays."""
        Xb = _f64(Xb)
        if Xb.ndim != 2 or Xb.shape[1] != self.d:
            raise Exception("x does not have the right size!")
        B = Xb.shape[0]
        dmu, dmse = np.empty((B, self.d)), np.empty((B, self.d))
        self._check(self._lib.bogp_gradient_batch(self._h, _ptr(Xb), B, _ptr(dmu), _ptr(dmse)))
        return dmu, dmse

    # -- multi-GPU exchange (bogp_comm.hip; one process per GPU) ---------------------------------------------
    def comm_init(self, comm_id: bytes, rank: int, world: int):
        """RCCL communicator over `world` handles (one per process / GPU); `comm_id` = comm_unique_id() of ONE rank."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("comm_id must be %d bytes" % COMM_ID_BYTES)
        self._check(self._lib.bogp_comm_init(self._h, comm_id, int(rank), int(world)))
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_attach(self, nccl_comm_ptr: int):
        self._check(self._lib.bogp_comm_attach(self._h, C.c_void_p(int(nccl_comm_ptr))))
        self.comm_rank, self.comm_world = self.comm_info()

    def comm_info(self) -> Tuple[int, int]:
        """(rank, world); world == 0 when the handle has no communicator."""
        r, w = C.c_int(), C.c_int()
        self._check(self._lib.bogp_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_destroy(self):
        self._check(self._lib.bogp_comm_destroy(self._h))
        self.comm_rank, self.comm_world = 0, 0

    def exchange_argmax(self, q: int, index_offset: int = 0, with_points: bool = True):
        """After sweep(): the global winners over all ranks' shards, identical on every rank:
        (best_val (q,), best_global_idx (q,), best_x (q, d) or None).  ONE ncclAllGather on device records."""
        if int(q) != self.__dict__.get("_last_q", -1):  # the C side packs ITS q records: a mismatch would under- or overrun these buffers
            raise ValueError("exchange_argmax(q=%d) does not follow a sweep of q = %d criteria on the current candidates" % (q, self.__dict__.get("_last_q", 0)))
        best, gidx = np.empty(q), np.empty(q, dtype=np.int64)
        x = np.empty((q, self.d)) if with_points else None
        self._check(self._lib.bogp_exchange_argmax(self._h, int(index_offset), _ptr(best), gidx.ctypes.data_as(_lp), _ptr(x)))
        return best, gidx, x

    def exchange_topk(self, q: int, k: int, index_offset: int = 0, with_points: bool = True):
        """After sweep_topk(): (values (q, k), global indices (q, k), points (q, k, d) or None), identical on every rank."""
        if (int(q), int(k)) != self.__dict__.get("_last_topk", (-1, -1)):
            raise ValueError("exchange_topk(q=%d, k=%d) does not follow a sweep_topk of that shape on the current candidates" % (q, k))
        best, gidx = np.empty((q, k)), np.empty((q, k), dtype=np.int64)
        x = np.empty((q, k, self.d)) if with_points else None
        self._check(self._lib.bogp_exchange_topk(self._h, int(index_offset), _ptr(best), gidx.ctypes.data_as(_lp), _ptr(x)))
        return best, gidx, x

    def last_timing(self) -> dict:
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        n = C.c_int()
        cast = lambda x: C.cast(C.byref(x), _dp)  # noqa: E731
        self._check(self._lib.bogp_last_timing(self._h, cast(a), cast(b), cast(c), C.cast(C.byref(n), _ip)))
        return dict(corr_ms=a.value, contract_ms=b.value, acquisition_ms=c.value, n_chunks=n.value)

    def set_prune(self, on=True):
        """Pruned sweep for this engine: sweep() without return_values skips the variance contraction of candidates that cannot win;
        winners and values are unchanged.  True (the default): automatic -- one bounding pass where it applies, else chunk by chunk;
        "chunks": always chunk by chunk; False: off."""
        if isinstance(on, str):
            if on != "chunks":
                raise ValueError('set_prune: %r is none of False, True, "chunks"' % (on,))
            mode = 2
        else:
            mode = int(bool(on))
        self._check(self._lib.bogp_set_prune(self._h, mode))

    def last_prune_path(self):
        """(path, survivors, rounds) of the last sweep: path is one of PRUNE_PATH_*; survivors behind the pilot and the rounds they
        were contracted in, for the one-pass paths."""
        path, rounds, surv = C.c_int(), C.c_int(), C.c_int64()
        self._check(self._lib.bogp_last_prune_path(self._h, C.cast(C.byref(path), _ip), C.cast(C.byref(surv), _lp), C.cast(C.byref(rounds), _ip)))
        return int(path.value), int(surv.value), int(rounds.value)

    def set_prune_bound32(self, on=True):
        """FP32 bounding stage of the one-pass pruned sweep (on by default): the bounding pass runs in FP32 with a proven margin per
        row, the exact FP64 pass only on the rows it cannot rule out.  Winners, values, survivors and paths are unchanged."""
        self._check(self._lib.bogp_set_prune_bound32(self._h, int(bool(on))))

    def last_bound32(self):
        """(rows bounded in FP32, rows kept over the segments, segments that ran the exact pass over all rows) of the last sweep."""
        rows, kept, fb = C.c_int64(), C.c_int64(), C.c_int()
        self._check(self._lib.bogp_last_bound32(self._h, C.cast(C.byref(rows), _lp), C.cast(C.byref(kept), _lp), C.cast(C.byref(fb), _ip)))
        return int(rows.value), int(kept.value), int(fb.value)

    def debug_bound32(self):
        """Per row of the last segment the FP32 stage bounded: (mu32, e_mu, wd32, e_w, flags) -- the FP32 sums r . gamma and w . r, their
        margins, the stage's flag; empty arrays where the stage did not run."""
        n = C.c_int64()
        self._check(self._lib.bogp_debug_bound32(self._h, 0, None, None, None, None, None, C.cast(C.byref(n), _lp)))
        n = int(n.value)
        out = [np.empty(n) for _ in range(4)]
        flags = np.empty(n, dtype=np.uint8)
        if n:
            m = C.c_int64()
            self._check(self._lib.bogp_debug_bound32(self._h, n, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                                                     flags.ctypes.data_as(C.POINTER(C.c_ubyte)), C.cast(C.byref(m), _lp)))
        return out[0], out[1], out[2], out[3], flags

    def last_contracted_rows(self) -> int:
        """Candidates that went through the variance contraction in the last predict() / sweep() (waits for a queued sweep)."""
        n = C.c_int64()
        self._check(self._lib.bogp_last_contracted_rows(self._h, C.cast(C.byref(n), _lp)))
        return int(n.value)

    def set_contract_tile(self, rows=0):
        """Candidates per workgroup of the direct variance contraction: 0 (the default) chooses per launch, 16 / 32 / 64 force one tile
        for this engine (tests and A/B).  No output bit depends on it."""
        if rows not in (0, 16, 32, 64):
            raise ValueError("set_contract_tile: %r is none of 0 (automatic), 16, 32, 64" % (rows,))
        self._check(self._lib.bogp_set_contract_tile(self._h, int(rows)))

    def last_contract_tile(self) -> int:
        """Tile rows (16, 32 or 64) of the last contraction launch of this engine."""
        n = C.c_int()
        self._check(self._lib.bogp_last_contract_tile(self._h, C.cast(C.byref(n), _ip)))
        return int(n.value)

    def selftest_gemm(self, A, B, C_in=None, ta=False, tb=False, alpha=1.0, beta=0.0, tri=0, split=True):
        """alpha op(A) op(B) + beta C through k_gemm64 (kernels_gemm.hip); A, B, C_in Fortran-ordered 2-D float64 arrays."""
        A = np.asfortranarray(A, dtype=np.float64)
        B = np.asfortranarray(B, dtype=np.float64)
        m, k = (A.shape[1], A.shape[0]) if ta else A.shape
        k2, n = (B.shape[1], B.shape[0]) if tb else B.shape
        if k != k2:
            raise ValueError("inner dimensions differ: %d vs %d" % (k, k2))
        out = np.zeros((m, n), order="F") if C_in is None else np.asfortranarray(C_in, dtype=np.float64).copy(order="F")
        self._check(self._lib.bogp_selftest_gemm(self._h, int(ta), int(tb), m, n, k, float(alpha), _ptr(A), A.shape[0], _ptr(B), B.shape[0],
                                                 float(beta), _ptr(out), out.shape[0], int(tri), int(split)))
        return out

    def flops_per_candidate(self) -> float:
        return float(self._lib.bogp_flops_per_candidate(self._h))

    def selftest_profile(self, what, arg, kernel=0, pexp=0.0):
        """`what` (SELFTEST_*) of every entry of `arg` on the device: the radial profile of `kernel`, K_pexp or 1 / Gamma exactly as the
        producers evaluate them per pair (csrc/bogp_device.h).  The *_PAIRS selectors take an (n, 2) array of (order, argument) rows."""
        arg = np.ascontiguousarray(arg, dtype=np.float64)
        n = arg.shape[0] if what >= SELFTEST_BESSEL_K_PAIRS else arg.size
        if what >= SELFTEST_BESSEL_K_PAIRS and (arg.ndim != 2 or arg.shape[1] != 2):
            raise ValueError("the *_PAIRS selectors take an (n, 2) array")
        out = np.empty(n)
        self._check(self._lib.bogp_selftest_profile(self._h, int(what), int(kernel), float(pexp), _ptr(arg), n, _ptr(out)))
        return out

    def selftest_criteria(self, what, *columns):
        """`what` (CRITERIA_*) of every row on the device: the scalar criterion functions of csrc/bogp_device.h themselves (ndtr, norm_pdf,
        ehvi_G, acq_value, feasibility, acq_upper_bound, acq_upper_bound_interval, prune_below), one row of arguments each.  `columns`:
        the function's arguments in order, scalars or arrays, broadcast against each other (bogp_selftest_criteria's columns)."""
        if not 1 <= len(columns) <= CRITERIA_COLUMNS:
            raise ValueError("between 1 and %d argument columns" % CRITERIA_COLUMNS)
        cols = np.broadcast_arrays(*[np.asarray(c, dtype=np.float64).ravel() for c in columns])
        rows = np.zeros((len(cols[0]), CRITERIA_COLUMNS))
        for k, c in enumerate(cols):
            rows[:, k] = c
        out = np.empty(len(rows))
        self._check(self._lib.bogp_selftest_criteria(self._h, int(what), _ptr(rows), len(rows), _ptr(out)))
        return out
