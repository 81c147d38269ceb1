"""ctypes binding of libmpcqp.so (the C ABI declared in include/mpcqp.h).

The library is built in-tree by ``__graft_entry__.build()`` (or
``make -C model_predictive_control_amd/csrc``) into
``model_predictive_control_amd/lib/libmpcqp.so``.  There is no fallback: if the
library is missing, or no GPU is present when a kernel is called, the call
raises -- the product path never silently drops to a CPU implementation.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPCQP_LIB", os.path.join(_HERE, "lib", "libmpcqp.so"))

F64 = 0
F32 = 1
TV = 1
GAM_PACKED = 8  # mpcqp_condense: Gam as its lower block triangle
IPM = 2
STRICT = 4
LOOP_COLD = 16  # mpcqp_mpc_poly_loop, mpcqp_mpc_box_loop_affine: every step from an empty active set
STATUS_POLISHED = 1 << 24
STATUS_UNREFINED = 1 << 25
STATUS_SOFTENED = 1 << 26  # mpcqp_mpc_poly_loop_soft: the step ends with a soft-active row
SQP_DONE = 1
SQP_EXACT = 2
SQP_FAIL = 4
SQP_PROJ = 8
SQP_HESS = {"gauss-newton": 0, "exact": 1, "exact-raw": 2}  # MPCQP_SQP_HESS_*
MODEL_FE = 0
MODEL_RK4 = 1
PLANT_FE = 0
PLANT_RK4 = 1
PLANT_RK4_SUB = 2

STATUS_OPTIMAL = 0
STATUS_MAXITER = 1
STATUS_NOT_CONVEX = 2
STATUS_INFEASIBLE = 3
STATUS_NONFINITE = 4
STATUS_NAMES = {0: "optimal", 1: "max_iter", 2: "not_convex", 3: "infeasible", 4: "nonfinite"}

# Every symbol include/mpcqp.h declares: the return kind, then one letter per
# argument in the prototype's order (blanks only group them: "pl" is a pointer
# with its instance stride).  tests/test_abi.py checks each entry against the
# header's prototype.
_KINDS = {"i": ctypes.c_int, "l": ctypes.c_int64, "z": ctypes.c_size_t, "d": ctypes.c_double,
          "p": ctypes.c_void_p, "s": ctypes.c_char_p, "D": ctypes.POINTER(ctypes.c_double),
          "F": ctypes.POINTER(ctypes.c_float)}
_TABLE = {
    "mpcqp_abi_version": "i",
    "mpcqp_last_error": "s",
    "mpcqp_max_box_n": "i i",
    "mpcqp_condense": "i iiiiii pl pl pl pl pl pl pl ppppppp",
    "mpcqp_solve_box": "i iii pl pl pl pl ppid p",
    "mpcqp_solve_box_vjp": "i iii pl ppl pl pppppppp",
    "mpcqp_mpc_box": "i iiiiii pl pl pl pl pl pl pl pl pl ppid p",
    "mpcqp_solve_poly_workspace": "l iiiii",
    "mpcqp_solve_poly": "i iiii ppl pppl pppppid pl p",
    "mpcqp_poly_workspace": "l iiiii",
    "mpcqp_poly_setup": "i iiiii ppppl p",
    "mpcqp_poly_solve": "i iiiiii ppl pl ppl pppppid p",
    "mpcqp_max_qp_size": "i i",
    "mpcqp_solve_qp": "i iiii pl pl pl ppl pl pl pppid p",
    "mpcqp_solve_qp_workspace": "z iiii",
    "mpcqp_sweep": "i iiii pl pl pi pp",
    "mpcqp_solve_qp_ws": "i iiii pl pl pl ppl pl pl pppid pz p",
    "mpcqp_solve_box_ws": "i iii pl pl pl pl ppid pz p",
    "mpcqp_mpc_qp_workspace": "z iiiiii",
    "mpcqp_mpc_qp": "i iiiiii pl pl pl pl pl pl pl ppl pl pl ppppid pz p",
    "mpcqp_mpc_ipm_workspace": "z iiiii",
    "mpcqp_mpc_ipm": "i iiiiii pl pl pl pl pl pl pl ppl pl pl pl pl pl pppppppiid pz p",
    "mpcqp_mpc_box_loop": "i iiiiii pl pl pl pl pl pl pl ppppid p",
    "mpcqp_mpc_box_loop_affine": "i iiiiiii pl pl pl pl pl pl pl pl pppppid p",
    "mpcqp_mpc_box_loop_vjp": "i iiiiii pl pl pl pl pl pl ppppppppppppppppp",
    "mpcqp_mpc_poly_loop": "i iiiiiiiii pppppl ppl ppppppppid p",
    "mpcqp_mpc_poly_loop_soft": "i iiiiiiiii pppppl ppl pppppppppppid p",
    "mpcqp_mpc_poly_loop_affine_workspace": "z iiiiiii",
    "mpcqp_mpc_poly_loop_affine": "i iiiiiiiii pppppl ppl ppppppl pl pz ppppppid p",
    "mpcqp_mpc_qp_profile": "i i",
    "mpcqp_mpc_qp_stage_ms": "i F",
    "mpcqp_bicycle_hessian": "i iiidDi ppppppppp",
    "mpcqp_bicycle_hessian_convex": "i iiidDi ppppppppd ppp",
    "mpcqp_bicycle_linearise": "i iiidDi pl pl ppppp",
    "mpcqp_bicycle_sqp_step": "i iiidDi pl pppppl ppl pppppppppppppd p",
    "mpcqp_bicycle_sqp_solve_workspace": "z ii",
    "mpcqp_bicycle_sqp_solve": "i iiidDii pl pppppl ppl pppppppppppiid pz p",
    "mpcqp_bicycle_mpc_loop": "i iiiidDiiDii pppppl ppl pppppppppiiidd pppppppz p",
    "mpcqp_bicycle_plant": "i iidDii ppl ppp",
    "mpcqp_sqp_shift": "i iii pppppppd p",
    "mpcqp_riccati": "i iiiii pl pl pl pl pl ppp",
    "mpcqp_bicycle_rti": "i iiidD pl pl ppppp",
    "mpcqp_gemv": "i iiiid pl pld pl p",
    "mpcqp_rollout": "i iiiii pppppp",
}
SIGNATURES = {name: (_KINDS[s[0]], [_KINDS[c] for c in s[1:].replace(" ", "")])
              for name, s in _TABLE.items()}

# The symbols of include/mpcqp_diff.h, in the same notation
# (tests/test_condense_vjp_host.py checks them against that header).
_TABLE_DIFF = {
    "mpcqp_condense_vjp": "i iiiiii pl pl pl pl pl pl pl ppp ppppppp p p",
}
SIGNATURES_DIFF = {name: (_KINDS[s[0]], [_KINDS[c] for c in s[1:].replace(" ", "")])
                   for name, s in _TABLE_DIFF.items()}

# The symbols of include/mpcqp_poly_diff.h (tests/test_poly_vjp_host.py checks
# them against that header).
_TABLE_POLY_DIFF = {
    "mpcqp_poly_solve_vjp_workspace": "z iiiii",
    "mpcqp_poly_solve_vjp": "i iiiiii ppp pp pppp p pz p",
}
SIGNATURES_POLY_DIFF = {name: (_KINDS[s[0]], [_KINDS[c] for c in s[1:].replace(" ", "")])
                        for name, s in _TABLE_POLY_DIFF.items()}

# The symbols of include/mpcqp_poly_loop_diff.h (tests/test_poly_loop_vjp_host.py
# checks them against that header).
_TABLE_POLY_LOOP_DIFF = {
    "mpcqp_mpc_poly_loop_vjp_workspace": "z iiiiii",
    "mpcqp_mpc_poly_loop_vjp": "i iiiiiiii pppp pp pppp pppppp p pz p",
}
SIGNATURES_POLY_LOOP_DIFF = {name: (_KINDS[s[0]], [_KINDS[c] for c in s[1:].replace(" ", "")])
                             for name, s in _TABLE_POLY_LOOP_DIFF.items()}

ABI_VERSION = 1

_lock = threading.Lock()
_lib = None


class MpcqpError(RuntimeError):
    """A libmpcqp entry point returned a negative code."""


def load(path: str | None = None):
    """Load (once) and return the ctypes library; raise if it is missing."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise ImportError(
                f"libmpcqp.so not found at {p}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP path has no CPU fallback)")
        lib = ctypes.CDLL(p)
        for name, (res, args) in (*SIGNATURES.items(), *SIGNATURES_DIFF.items(),
                                  *SIGNATURES_POLY_DIFF.items(),
                                  *SIGNATURES_POLY_LOOP_DIFF.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        v = lib.mpcqp_abi_version()
        if v != ABI_VERSION:
            raise ImportError(f"libmpcqp ABI {v} != expected {ABI_VERSION}")
        if path is None:
            _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mpcqp_last_error().decode(errors="replace")
        raise MpcqpError(f"{what} failed ({rc}): {msg}")
