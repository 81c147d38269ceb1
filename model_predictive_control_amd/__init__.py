"""MI355X-native batched condensed-QP MPC solver.

A drop-in for the receding-horizon inner loop of
konnpaku-youmu/Model_Predictive_Control: the reference's Python call
surfaces (session_1/FHC.py, session_1/LinearSystem.py,
session_1/session1_sol.py, session_4/main.py ``MPCController``) are kept, and
the per-step work -- condense (A, B) over the horizon into H, F, f, then solve
the box / polytope QP -- runs as hand-written gfx950 HIP kernels behind the
C ABI of include/mpcqp.h (libmpcqp.so, loaded with ctypes).

Submodules:
  batched        device API on torch tensors (condense, solve_box, solve_poly,
                 riccati, gemv, rollout)
  fhc            FHC.py surface (ricatti_recursion, AutoCruising, ...)
  linear_system  LinearSystem.py surface
  session1       session1_sol.py surface
  problems       session 2/3 problem data + ControllerLog
  parameters     VehicleParameters (session_4/parameters.py)
  bicycle        kinematic bicycle, integrators, batched FE linearisation
  mpc            MPCController (session_4/main.py) on device
  distributed    batch sharding / gather across GPUs
  autograd       solve_box_diff, mpc_box_diff: the box QP and the fused box-MPC
                 step as torch.autograd functions; box_loop_diff,
                 mpc_box_loop_diff: the one-launch box-MPC episode with a
                 one-launch backward; condense_diff, mpc_box_model_diff,
                 mpc_box_loop_model_diff: the same with gradients of the
                 prediction model A, B, c; poly_solve_diff, mpc_poly_diff: the
                 polytope QP and the state-constrained MPC step;
                 poly_loop_diff, mpc_poly_loop_diff: the one-launch
                 state-constrained episode with a one-launch backward (all
                 eleven also exported here)
  condense_diff  condense_vjp: the adjoint of condensing on the device
  poly_diff      poly_solve_vjp, shared_grads: the adjoint of the polytope QP;
                 poly_loop_vjp, loop_shared_grads: that of its one-launch loop
"""
from . import _native  # noqa: F401

__version__ = "0.1.0"

_AUTOGRAD = ("solve_box_diff", "mpc_box_diff", "box_loop_diff", "mpc_box_loop_diff",
             "condense_diff", "mpc_box_model_diff", "mpc_box_loop_model_diff",
             "poly_solve_diff", "mpc_poly_diff", "poly_loop_diff", "mpc_poly_loop_diff")
__all__ = ["library_path", *_AUTOGRAD]


def __getattr__(name):
    # the autograd entry points, resolved on first use so that importing
    # the package stays free of torch
    if name == "condense_diff":
        # also the name of a submodule: the module itself, which is callable
        # as autograd.condense_diff, so the name is one object either way
        import importlib

        return importlib.import_module(".condense_diff", __name__)
    if name in _AUTOGRAD:
        from . import autograd

        return getattr(autograd, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def library_path() -> str:
    return _native.LIB_PATH
