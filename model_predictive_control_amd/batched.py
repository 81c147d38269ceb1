"""Batched device API over libmpcqp (torch tensors on the GPU).

This is the layer the reference-shaped surfaces (``fhc``, ``linear_system``,
``session1``, ``mpc``) and ``bench.py`` call.  Every function enqueues HIP
kernels on torch's current stream through the C ABI of include/mpcqp.h; no
computation happens on the host.

Shape conventions (batch-outermost, row-major):

* a per-instance input carries a leading batch dimension, a shared input
  does not (it is passed with stride 0);
* ``z`` is stage-major  [u_0; ...; u_{N-1}]  (session_4/main.py:46,110);
* symmetric matrices (H) are packed lower, n(n+1)/2 per instance
  (``pack_lower`` / ``unpack_lower`` convert).
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native as nat

__all__ = [
    "condense", "solve_box", "solve_box_vjp", "mpc_box", "mpc_box_loop", "mpc_box_loop_vjp",
    "mpc_poly_loop", "tracking_terms", "mpc_qp", "mpc_ipm", "solve_poly", "solve_qp", "sweep",
    "riccati", "gemv", "rollout", "bicycle_rti", "bicycle_linearise", "bicycle_hessian",
    "bicycle_sqp_step", "pack_lower", "unpack_lower", "status_code", "status_iters",
    "workspace_bytes",
]


# ------------------------------------------------------------- marshalling
# Everything between a wrapper's Python operands and its C call.  The wrappers
# reach _lib, _stream, _dev and _workspace through the module's globals, so a
# replacement assigned to one of these names takes effect (tools/ab_libs.py,
# tests/_batched_record.py).  Nothing here reads device memory or synchronises:
# shapes, dtypes, strides and data_ptr() only, so the wrappers can be captured
# into a HIP graph.
def _lib():
    return nat.load()


def _code(dtype: torch.dtype) -> int:
    if dtype == torch.float64:
        return nat.F64
    if dtype == torch.float32:
        return nat.F32
    raise TypeError(f"libmpcqp supports float64/float32, got {dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


_WS: dict = {}


def _workspace(nbytes: int, dev, ws: torch.Tensor | None = None) -> torch.Tensor | None:
    """Device scratch of the two-kernel QP path (swept matrix, s0, hand-off
    counter and list).

    * ``ws`` given: the caller's buffer is used as is (checked for size).
    * inside a HIP-graph capture: a fresh buffer, which the graph's private
      pool keeps for the graph's lifetime; never a cached one, so a later
      resize of the cache cannot pull memory out from under a captured graph.
    * otherwise: one grow-only buffer per (device, stream).  Kernels on one
      stream run in order, so solves on the same stream may share it; solves
      on different streams get different buffers.  Growing drops the smaller
      buffer (the caching allocator reuses it stream-ordered on that stream).
    """
    if nbytes <= 0:
        return None
    if ws is not None:
        if ws.device.type != "cuda" or ws.numel() * ws.element_size() < nbytes:
            raise ValueError(f"workspace must be a device buffer of >= {nbytes} bytes")
        return ws
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        _WS.pop(key, None)
        buf = _WS[key] = torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)
    return buf


def workspace_bytes(dtype: torch.dtype, batch: int, n: int, m: int = 0) -> int:
    """Bytes of the ``ws=`` buffer solve_box (m = 0) / solve_qp need."""
    return int(_lib().mpcqp_solve_qp_workspace(_code(dtype), batch, n, m))


def _dev(x, dtype, device):
    if x is None:
        return None
    t = torch.as_tensor(x, dtype=dtype, device=device)
    if t.device.type != "cuda":
        raise ValueError("libmpcqp needs CUDA(HIP) tensors")
    return t.contiguous()


def _inst(t, base_ndim: int, name: str):
    """(stride, batch) of an input that is shared (ndim == base) or batched."""
    if t is None:
        return 0, None
    if t.ndim == base_ndim:
        return 0, None
    if t.ndim == base_ndim + 1:
        b = int(t.shape[0])
        if b == 0:      # what indexing the first instance of an empty batch raises
            raise IndexError("index 0 is out of bounds for dimension 0 with size 0")
        return t.numel() // b, b
    raise ValueError(f"{name}: expected {base_ndim} or {base_ndim + 1} dims, got {tuple(t.shape)}")


def _batch_of(*pairs):
    bs = {b for _, b in pairs if b is not None}
    if len(bs) > 1:
        raise ValueError(f"inconsistent batch sizes {sorted(bs)}")
    return bs.pop() if bs else 1


def _inst_one(t, base_ndim: int, name: str, when: bool = True):
    """``_inst`` where a leading dimension of 1 counts as shared if ``when``
    (a shared plant condenses to one instance)."""
    s, b = _inst(t, base_ndim, name)
    return (0, None) if b == 1 and when else (s, b)


def _dt_dev(A):
    """(dtype, device) of a call, from its leading operand."""
    dt = A.dtype if isinstance(A, torch.Tensor) else torch.float64
    dev = A.device if isinstance(A, torch.Tensor) else torch.device("cuda")
    return dt, dev


def _weight_r(R, nu: int):
    """R as (nu, nu) (or batched).  FHC.py:141 passes R with shape (1,), which
    NumPy broadcasts; a 1-D R is accepted only for nu == 1 (shape (1,)) -- a
    vector of diagonal weights must be given as a matrix (torch.diag)."""
    if R.ndim == 1:
        if R.shape[0] != 1 or nu != 1:
            raise ValueError(f"R of shape {tuple(R.shape)} with nu={nu}: pass an (nu, nu) matrix")
        return R.reshape(1, 1).contiguous()
    return R


def _plant(A, B, Q, R, Qf, x0, c, tv: bool):
    """The plant operands of condense / mpc_box / mpc_qp / mpc_ipm, converted:
    returns (dt, dev, nx, nu, keep, insts, head).  ``keep`` holds the tensors
    (A, B, Q, R, Qf, c, x0) -- ``_dev`` may have made copies that nothing else
    references -- so a wrapper holds on to it until its C call has returned.
    ``insts`` are their (stride, batch) pairs and ``head`` the 14 values
    ``ptr(A), sA, .. ptr(c), sC, ptr(x0), sX`` of the C prototypes."""
    dt, dev = _dt_dev(A)
    A, B, Q, R, Qf, x0, c = [_dev(v, dt, dev) for v in (A, B, Q, R, Qf, x0, c)]
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    R = _weight_r(R, nu)
    base = 3 if tv else 2
    keep = (A, B, Q, R, Qf, c, x0)
    insts = (_inst(A, base, "A"), _inst(B, base, "B"), _inst(Q, 2, "Q"), _inst(R, 2, "R"),
             _inst(Qf, 2, "Qf"), _inst(c, 2, "c"), _inst(x0, 1, "x0"))
    head = []
    for t, (s, _) in zip(keep, insts):
        head += (None if t is None else t.data_ptr(), s)
    return dt, dev, nx, nu, keep, insts, head


def _bound(v, n, dt, dev):
    """(tensor, stride, batch) of a box bound: None, a scalar (Python number or
    0-d tensor, filled to (n,)), shared or per instance."""
    if v is None:
        return None, 0, None
    if not isinstance(v, torch.Tensor) and (isinstance(v, (int, float))):
        return torch.full((n,), float(v), dtype=dt, device=dev), 0, None
    t = _dev(v, dt, dev)
    if t.ndim == 0:
        return t.expand(n).contiguous(), 0, None
    return (t, *_inst(t, 1, "bound"))


def _alloc(spec: dict, dev, out=None, *, keyed: bool = False, check: bool = False):
    """The output tensors of a call.  ``spec`` maps each output's name, in the
    order of the result, to (shape, dtype), or to None for one that is not
    produced.  ``keyed``: ``out`` is a dict (or None) and the result a copy of
    it with the missing outputs allocated; otherwise ``out`` is a sequence in
    the order of ``spec``, returned as it is, and None allocates them all.
    ``check``: what the caller supplied must be contiguous with the shape and
    dtype of ``spec`` (sequence form: also tensors on ``dev``, and as many as
    ``spec`` has); without it the caller's objects are passed on unexamined."""
    if keyed or out is None:
        o = dict(out or {}) if keyed else {}
        for k, v in spec.items():
            if k not in o:
                o[k] = None if v is None else torch.empty(v[0], dtype=v[1], device=dev)
            elif check and (o[k].shape != v[0] or o[k].dtype != v[1] or not o[k].is_contiguous()):
                raise ValueError(f"out[{k!r}] must be a contiguous {v[1]} tensor of shape {v[0]}")
        return o if keyed else tuple(o.values())
    if not check:
        return out
    if not isinstance(out, (tuple, list)) or len(out) != len(spec):
        raise ValueError(f"out must be a triple ({', '.join(spec)})")
    for t, (name, (shp, kd)) in zip(out, spec.items()):
        if (not isinstance(t, torch.Tensor) or t.shape != shp or t.dtype != kd or t.device != dev
                or not t.is_contiguous()):
            raise ValueError(f"out {name} must be a contiguous {kd} tensor of shape {shp} on {dev}")
    return tuple(out)


def _row_pair(lo, hi, policy: str, side, mixed: str = ""):
    """A lower/upper pair of bounds that the C call reads with ONE instance
    stride.  ``side(t, k)`` validates one side (k = 0 lower, 1 upper; t may be
    None) with its caller's message and returns (tensor, stride, batch).  Where
    one side is shared and the other per instance, ``policy`` decides:

    * "broadcast": both are expanded to the per-instance shape, so the shared
      stride is never applied to a per-instance buffer or the reverse (which
      would read past the shared side's end);
    * "raise": ValueError(``mixed``), ``{lo}`` and ``{hi}`` being the shapes;
    * "equal": the shapes must be equal to begin with, else ValueError(``mixed``)
      before either side is looked at.

    Returns (lo, hi, stride, batch of lo, batch of hi)."""
    both = lo is not None and hi is not None
    if policy == "equal" and both and lo.shape != hi.shape:
        raise ValueError(mixed)
    lo, sl, bl = side(lo, 0)
    hi, su, bu = side(hi, 1)
    if policy == "raise" and both and (bl is None) != (bu is None):
        raise ValueError(mixed.format(lo=tuple(lo.shape), hi=tuple(hi.shape)))
    if policy == "broadcast" and (bl is not None or bu is not None):
        shape = (lo if bl is not None else hi).shape
        lo, hi = (None if v is None else v.expand(shape).contiguous() for v in (lo, hi))
    return lo, hi, max(sl, su), bl, bu


def _bound_pair(lo, hi, b: int, width: int, what: str):
    """The bound pairs of the bicycle entry points: each side None, (width,)
    shared or (b, width); a shared side next to a per-instance one is
    broadcast to (b, width) (``_row_pair``).  Returns (lo, hi, stride)."""
    def side(v, _):
        if v is None:
            return None, 0, None
        if tuple(v.shape) not in ((width,), (b, width)):
            raise ValueError(f"{what}: shape {tuple(v.shape)} is neither ({width},) nor ({b}, {width})")
        return (v, width, b) if v.ndim == 2 else (v, 0, None)

    return _row_pair(lo, hi, "broadcast", side)[:3]


def _bike_params(params):
    return (ctypes.c_double * 4)(params.axis_front, params.axis_rear, params.acceleration,
                                 params.friction)


def _sqp_state(state: dict):
    """The pointer run (rho, kkt, mu, flags, fix) of the bicycle SQP state."""
    return (_ptr(state["rho"]), _ptr(state["kkt"]), _ptr(state["mu"]), _ptr(state["flags"]),
            _ptr(state.get("fix")))


def _check_tensors(who: str, dev, specs):
    """Each (name, tensor, shape, dtype) of ``specs`` is contiguous, of that
    shape and dtype, on ``dev``."""
    for name, t, shp, dt in specs:
        if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {name} must be a contiguous {dt} device tensor of shape {shp}")


def status_code(status: torch.Tensor) -> torch.Tensor:
    return status & 0xFF


def status_iters(status: torch.Tensor) -> torch.Tensor:
    return (status >> 8) & 0xFFFF


# ----------------------------------------------------------------- packing
def _tril_index(n: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    r, c = torch.tril_indices(n, n, device=device)
    return r, c


def pack_lower(H: torch.Tensor) -> torch.Tensor:
    """(..., n, n) symmetric -> (..., n(n+1)/2) row-major packed lower."""
    n = H.shape[-1]
    r, c = _tril_index(n, H.device)
    return H[..., r, c].contiguous()


def unpack_lower(P: torch.Tensor, n: int) -> torch.Tensor:
    """(..., n(n+1)/2) packed lower -> (..., n, n) symmetric."""
    r, c = _tril_index(n, P.device)
    out = P.new_zeros(P.shape[:-1] + (n, n))
    out[..., r, c] = P
    out[..., c, r] = P
    return out


# ---------------------------------------------------------------- condense
def condense(A, B, Q, R, Qf, N: int, x0=None, c=None, *, tv: bool = False,
             outputs=("H", "f"), out: dict | None = None, gam_packed: bool = False) -> dict:
    """Batched condensing (include/mpcqp.h ``mpcqp_condense``).

    A: (nx,nx) | (b,nx,nx) | with ``tv``: (N,nx,nx) | (b,N,nx,nx); B likewise
    with nu columns; Q/Qf (nx,nx) | (b,nx,nx); R (nu,nu) | (b,nu,nu);
    x0 (nx,) | (b,nx); c (N,nx) | (b,N,nx).  Returns a dict with the requested
    ``outputs`` among H (packed), F, f, Gam, Phi, xbar.  ``gam_packed``: Gam
    as its lower block triangle, (b, nx*nu*N*(N+1)/2) (``MPCQP_GAM_PACKED``;
    ``unpack_gam`` restores the dense (b, N*nx, N*nu) form).
    """
    dt, dev, nx, nu, keep, insts, head = _plant(A, B, Q, R, Qf, x0, c, tv)
    batch = _batch_of(*insts)
    n = N * nu
    want = set(outputs) | {"H"}
    out = out or {}
    shapes = {"H": (batch, n * (n + 1) // 2), "F": (batch, n, nx), "f": (batch, n),
              "Gam": (batch, nx * nu * N * (N + 1) // 2) if gam_packed else (batch, N * nx, n),
              "Phi": (batch, N * nx, nx), "xbar": (batch, N * nx)}
    out = _alloc({k: (shapes[k], dt) for k in want if k not in out}, dev, out, keyed=True)
    rc = _lib().mpcqp_condense(
        _code(dt), batch, nx, nu, N, (nat.TV if tv else 0) | (nat.GAM_PACKED if gam_packed else 0),
        *head, *[_ptr(out.get(k)) for k in shapes], _stream())
    nat.check(rc, "mpcqp_condense")
    return {k: out[k] for k in want}


def unpack_gam(P, N: int, nx: int, nu: int):
    """Dense (..., N*nx, N*nu) Gamma from its packed lower block triangle
    (``condense(..., gam_packed=True)``): block row k holds its (k+1)*nu
    leading columns from offset nx*nu*k*(k+1)/2, column by column (entry
    (k*nx + q, col) at nx*nu*k*(k+1)/2 + col*nx + q)."""
    out = P.new_zeros(P.shape[:-1] + (N * nx, N * nu))
    for k in range(N):
        o, w = nx * nu * k * (k + 1) // 2, (k + 1) * nu
        out[..., k * nx:(k + 1) * nx, :w] = P[..., o:o + nx * w].reshape(P.shape[:-1] + (w, nx)).transpose(-1, -2)
    return out


# ---------------------------------------------------- fused condense + box
def mpc_box(A, B, Q, R, Qf, N: int, x0, lb=None, ub=None, c=None, *, tv: bool = False,
            max_iter: int = 0, tol: float = 0.0, out: tuple | None = None):
    """Fused per-instance condense + input-box QP (include/mpcqp.h
    ``mpcqp_mpc_box``).  Same plant conventions as ``condense``; lb/ub are
    scalars, (N*nu,) shared or (b, N*nu).  Returns (z (b, N*nu), status)."""
    dt, dev, nx, nu, keep, insts, head = _plant(A, B, Q, R, Qf, x0, c, tv)
    n = N * nu
    lbt, slb, blb = _bound(lb, n, dt, dev)
    ubt, sub, bub = _bound(ub, n, dt, dev)
    batch = _batch_of(*insts, (slb, blb), (sub, bub))
    z, status = _alloc({"z": ((batch, n), dt), "status": ((batch,), torch.int32)}, dev, out)
    rc = _lib().mpcqp_mpc_box(
        _code(dt), batch, nx, nu, N, nat.TV if tv else 0, *head, _ptr(lbt), slb, _ptr(ubt), sub,
        _ptr(z), _ptr(status), int(max_iter), float(tol), _stream())
    nat.check(rc, "mpcqp_mpc_box")
    return z, status


# --------------------------------------- fused condense + state/input box
def mpc_qp_workspace_bytes(dtype: torch.dtype, batch: int, nx: int, nu: int, N: int,
                           state_box: bool = True) -> int:
    """Bytes of the ``ws=`` buffer ``mpc_qp`` needs."""
    return int(_lib().mpcqp_mpc_qp_workspace(_code(dtype), batch, nx, nu, N, int(bool(state_box))))


def _mpc_step_args(A, B, Q, R, Qf, N, x0, xlo, xhi, lb, ub, c, tv):
    """Normalise the arguments shared by mpc_qp / mpc_ipm (plant conventions
    of ``condense``; state bounds (nx,) repeated over the horizon, (N*nx,)
    shared or (b, N*nx); input bounds as ``mpc_box``)."""
    dt, dev, nx, nu, keep, insts, head = _plant(A, B, Q, R, Qf, x0, c, tv)
    n, m = N * nu, N * nx

    def sbound(v, _):
        if v is None:
            return None, 0, None
        t = _dev(v, dt, dev)
        if t.ndim == 1 and t.shape[0] == nx and nx != m:
            t = t.repeat(N)
        s, bb = _inst(t, 1, "state bound")
        if t.shape[-1] != m:
            raise ValueError(f"state bounds need {m} (= N*nx) entries, got {tuple(t.shape)}")
        return t, s, bb

    xlo_t, xhi_t, sXb, bxl, bxh = _row_pair(
        xlo, xhi, "raise", sbound, "xlo and xhi must both be shared or both per instance")
    lbt, slb, blb = _bound(lb, n, dt, dev)
    ubt, sub, bub = _bound(ub, n, dt, dev)
    batch = _batch_of(*insts, (sXb, bxl), (sXb, bxh), (slb, blb), (sub, bub))
    return dict(dt=dt, dev=dev, nx=nx, nu=nu, n=n, m=m, batch=batch,
                head=(*head, _ptr(xlo_t), _ptr(xhi_t), sXb, _ptr(lbt), slb, _ptr(ubt), sub),
                keep=(keep, xlo_t, xhi_t, lbt, ubt),
                sbox=xlo_t is not None or xhi_t is not None)


def mpc_qp(A, B, Q, R, Qf, N: int, x0, xlo=None, xhi=None, lb=None, ub=None, c=None, *,
           tv: bool = False, states: bool = False, max_iter: int = 0, tol: float = 0.0,
           out: tuple | None = None, ws: torch.Tensor | None = None, ipm: bool = False):
    """One MPC step with input box and state box, end to end (include/mpcqp.h
    ``mpcqp_mpc_qp``): condense + QP, fp32 refined against the dynamics.
    Steps beyond the dense kernels' size (and every step with ``ipm=True``)
    run on the stage-wise interior point (``mpc_ipm``).

    Plant conventions as ``condense``; xlo/xhi: state bounds on x_1..x_N,
    (nx,) repeated over the horizon, (N*nx,) shared or (b, N*nx); lb/ub as
    ``mpc_box``.  Returns (z (b, N*nu), y (b, N*nx) or None, status[, X
    (b, N, nx) when ``states``]); y are the state-row multipliers (> 0 at xhi).
    """
    g = _mpc_step_args(A, B, Q, R, Qf, N, x0, xlo, xhi, lb, ub, c, tv)
    dt, dev, batch, n, m, nx = g["dt"], g["dev"], g["batch"], g["n"], g["m"], g["nx"]
    sbox = g["sbox"]
    o = _alloc({"z": ((batch, n), dt), "y": ((batch, m), dt) if sbox else None,
                "status": ((batch,), torch.int32), "X": ((batch, N, nx), dt) if states else None},
               dev, out)
    z, y, status = o[:3]
    X = o[3] if len(o) > 3 else None
    lib = _lib()
    wsb = int(lib.mpcqp_mpc_qp_workspace(_code(dt), batch, nx, g["nu"], N, int(sbox)))
    ws = _workspace(wsb, dev, ws)
    flags = (nat.TV if tv else 0) | (nat.IPM if ipm else 0)
    rc = lib.mpcqp_mpc_qp(_code(dt), batch, nx, g["nu"], N, flags, *g["head"],
                          _ptr(z), _ptr(y), _ptr(X), _ptr(status), int(max_iter), float(tol),
                          _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_mpc_qp")
    return (z, y, status, X) if states else (z, y, status)


def mpc_ipm(A, B, Q, R, Qf, N: int, x0, xlo=None, xhi=None, lb=None, ub=None, c=None, *,
            tv: bool = False, U0=None, H2=None, q2=None, max_iter: int = 0, tol: float = 0.0,
            strict: bool = False, skip=None, skip_mask: int = 0, out: dict | None = None,
            ws: torch.Tensor | None = None):
    """The MPC step of ``mpc_qp`` on the stage-wise interior point, any horizon
    (include/mpcqp.h ``mpcqp_mpc_ipm``; nx <= 4, nu <= 2).  U0: optional
    starting inputs (b, N, nu) or (b, N*nu).  H2 (b, N, nx+nu, nx+nu), q2
    (b, N, nx+nu): optional extra stage cost 1/2 w'H2 w + q2'w over
    w = [x_k; u_k] (may be indefinite).  Returns a dict with z (b, N*nu),
    X (b, N, nx) = x_1..x_N, y (b, N*nx) state-bound and lam_u (b, N*nu)
    input-bound multipliers (> 0 at the upper bound), pi (b, N, nx) costates
    of the dynamics, status (b,).  ``strict``: a non-positive pivot ends an
    instance with STATUS_NOT_CONVEX instead of regularising.  ``skip`` (b,)
    int32 with ``skip_mask``: instances with skip & skip_mask != 0 are left
    untouched.  ``out``: a dict of preallocated outputs."""
    g = _mpc_step_args(A, B, Q, R, Qf, N, x0, xlo, xhi, lb, ub, c, tv)
    dt, dev, batch, n, m, nx = g["dt"], g["dev"], g["batch"], g["n"], g["m"], g["nx"]
    U0t = None if U0 is None else _dev(U0, dt, dev).reshape(batch, n)
    n2 = nx + g["nu"]
    H2t = None if H2 is None else _dev(H2, dt, dev).reshape(batch, N * n2 * n2)
    q2t = None if q2 is None else _dev(q2, dt, dev).reshape(batch, N * n2)
    o = _alloc(dict(z=((batch, n), dt), y=((batch, m), dt), lam_u=((batch, n), dt),
                    X=((batch, N, nx), dt), pi=((batch, N, nx), dt),
                    status=((batch,), torch.int32)), dev, out, keyed=True)
    lib = _lib()
    wsb = int(lib.mpcqp_mpc_ipm_workspace(_code(dt), batch, nx, g["nu"], N))
    ws = _workspace(wsb, dev, ws)
    if skip is not None and (skip.dtype != torch.int32 or skip.shape != (batch,)
                             or skip.device != dev):
        raise ValueError("skip must be an int32 device tensor of shape (batch,)")
    flags = (nat.TV if tv else 0) | (nat.STRICT if strict else 0)
    rc = lib.mpcqp_mpc_ipm(_code(dt), batch, nx, g["nu"], N, flags, *g["head"],
                           _ptr(U0t), 0 if U0t is None else n, _ptr(H2t),
                           0 if H2t is None else N * n2 * n2, _ptr(q2t),
                           0 if q2t is None else N * n2, _ptr(o["z"]), _ptr(o["y"]), _ptr(o["X"]),
                           _ptr(o["lam_u"]), _ptr(o["pi"]), _ptr(o["status"]), _ptr(skip),
                           int(skip_mask) if skip is not None else 0, int(max_iter),
                           float(tol), _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_mpc_ipm")
    return o


def mpc_box_loop(A, B, Q, R, Qf, N: int, x0, lb=None, ub=None, steps: int = 1, *,
                 plans: bool = False, max_iter: int = 0, tol: float = 0.0,
                 condensed: dict | None = None, out: dict | None = None,
                 g=None, w=None, x_ref=None, u_ref=None, cold: bool = False) -> dict:
    """The receding-horizon loop of the input-box MPC on a linear plant, on
    the device (include/mpcqp.h ``mpcqp_mpc_box_loop``): for t < steps,
    z_t = argmin 1/2 z'Hz + (F x_t)'z over lb <= z <= ub, x_{t+1} = A x_t + B
    u_0(z_t) -- LinearSystem.simulate (LinearSystem.py:20-26) under the MPC
    policy of MPCController.solve (main.py:115-116).  A (nx,nx) | (b,nx,nx), B
    likewise; x0 (b, nx).  H and F come from ``condense`` of the same plant
    (once; pass ``condensed`` to reuse them).  Returns xs (steps+1, b, nx), us
    (steps, b, nu), status (steps, b), and with ``plans`` zs (steps, b, N*nu).

    ``g`` ((steps, n) shared by the batch, or (steps, b, n)) is a per-step
    linear term: the step's gradient is F x_t + g_t.  ``x_ref`` / ``u_ref``
    (shapes of ``tracking_terms``) build it from a reference trajectory
    instead, for which the plant is condensed with Gam as well (per instance
    when the plants are); passing both g and a reference is an error.  ``w``
    (steps, b, nx) is a plant disturbance, x_{t+1} = A x_t + B u_t + w_t.
    ``cold`` starts every step from the empty active set.  With any of these
    the call goes to ``mpcqp_mpc_box_loop_affine``."""
    dt, dev = _dt_dev(A)
    A, B = _dev(A, dt, dev), _dev(B, dt, dev)
    x0 = _dev(x0, dt, dev)
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    if x0.ndim != 2 or x0.shape[1] != nx:
        raise ValueError(f"x0 must be (batch, {nx}), got {tuple(x0.shape)}")
    batch, n, T = int(x0.shape[0]), N * nu, int(steps)
    tracking = x_ref is not None or u_ref is not None
    if tracking and g is not None:
        raise ValueError("mpc_box_loop: pass either g or a reference (x_ref / u_ref), not both")
    cd = dict(condensed or condense(A, B, Q, R, Qf, N,
                                    outputs=("H", "F", "Gam") if tracking else ("H", "F")))
    if tracking and "Gam" not in cd:
        cd["Gam"] = condense(A, B, Q, R, Qf, N, outputs=("Gam",))["Gam"]
    H, F = cd["H"], cd["F"]
    # H and F with a leading 1 are shared whatever the batch; A and B are taken as given
    sH, _ = _inst_one(H, 1, "H")
    sF, _ = _inst_one(F, 2, "F")
    sA, _ = _inst(A, 2, "A")
    sB, _ = _inst(B, 2, "B")
    lbt, slb, _ = _bound(lb, n, dt, dev)
    ubt, sub, _ = _bound(ub, n, dt, dev)
    if tracking:
        Gam = cd["Gam"]
        if Gam.ndim == 3 and Gam.shape[0] == 1:
            Gam = Gam[0]
        g = tracking_terms({"Gam": Gam}, _dev(Q, dt, dev), _weight_r(_dev(R, dt, dev), nu),
                           _dev(Qf, dt, dev), N, T, x_ref, u_ref)
    g, w = _dev(g, dt, dev), _dev(w, dt, dev)
    if g is not None and tuple(g.shape) not in ((T, n), (T, batch, n)):
        raise ValueError(f"g must be ({T}, {n}) or ({T}, {batch}, {n}), got {tuple(g.shape)}")
    if w is not None and tuple(w.shape) != (T, batch, nx):
        raise ValueError(f"w must be ({T}, {batch}, {nx}), got {tuple(w.shape)}")
    spec = dict(xs=((T + 1, batch, nx), dt), us=((T, batch, nu), dt),
                status=((T, batch), torch.int32))
    if plans:
        spec["zs"] = ((T, batch, n), dt)
    o = _alloc(spec, dev, out, keyed=True)
    dims = (_code(dt), batch, nx, nu, N, T)
    head = (_ptr(H), sH, _ptr(F), sF, _ptr(A), sA, _ptr(B), sB, _ptr(x0), nx, _ptr(lbt), slb,
            _ptr(ubt), sub)
    tail = (_ptr(o["xs"]), _ptr(o["us"]), _ptr(o.get("zs")), _ptr(o["status"]), int(max_iter),
            float(tol), _stream())
    if g is not None or w is not None or cold:
        rc = _lib().mpcqp_mpc_box_loop_affine(
            *dims, nat.LOOP_COLD if cold else 0, *head,
            _ptr(g), 0 if g is None or g.ndim == 2 else n, _ptr(w), *tail)
        nat.check(rc, "mpcqp_mpc_box_loop_affine")
        return o
    rc = _lib().mpcqp_mpc_box_loop(*dims, *head, *tail)
    nat.check(rc, "mpcqp_mpc_box_loop")
    return o


# ----------------------------------------------------------------- box QP
def solve_box(H, f, lb=None, ub=None, *, max_iter: int = 0, tol: float = 0.0,
              out: tuple | None = None, presweep: bool = True, ws: torch.Tensor | None = None):
    """Batched  min 1/2 z'Hz + f'z  s.t.  lb <= z <= ub.  Returns (z, status).
    ``ws``: optional caller-owned scratch (``workspace_bytes(dtype, batch, n)``).

    fp32 with n > 64: the -H^-1 sweep runs first as its own MFMA kernel
    (``mpcqp_solve_box_ws``) unless ``presweep=False``."""
    dt, dev = f.dtype, f.device
    f = _dev(f, dt, dev)
    H = _dev(H, dt, dev)
    n = int(f.shape[-1])
    if H.shape[-1] != n * (n + 1) // 2:
        raise ValueError(f"H must be packed lower with {n * (n + 1) // 2} entries, got {tuple(H.shape)}")
    sH, bH = _inst(H, 1, "H")
    sf, bf = _inst(f, 1, "f")
    lbt, slb, blb = _bound(lb, n, dt, dev)
    ubt, sub, bub = _bound(ub, n, dt, dev)
    batch = _batch_of((sH, bH), (sf, bf), (slb, blb), (sub, bub))
    z, status = _alloc({"z": ((batch, n), dt), "status": ((batch,), torch.int32)}, dev, out)
    lib = _lib()
    wsb = int(lib.mpcqp_solve_qp_workspace(_code(dt), batch, n, 0)) if presweep else 0
    ws = _workspace(wsb, dev, ws)
    rc = lib.mpcqp_solve_box_ws(_code(dt), batch, n, _ptr(H), sH, _ptr(f), sf, _ptr(lbt), slb,
                                _ptr(ubt), sub, _ptr(z), _ptr(status), int(max_iter), float(tol),
                                _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_solve_box_ws")
    return z, status


BOX_VJP_MAX_N = 32


def _vjp_common(lb, ub, n, dt, dev, batch, insts, status, status_shape):
    """What ``solve_box_vjp`` and ``mpc_box_loop_vjp`` share around their
    launch: the bounds (``_bound``, last dimension n), the batch consistency of
    ``insts`` ((stride, batch) pairs) and the bounds with ``batch``, and the
    forward's status.  Returns ``(lbt, slb, ubt, sub, status, shared)`` where
    ``shared(g, stride, ref=None)`` is the epilogue of a gradient: summed over
    the batch where the input is shared (stride 0), in the shape of ``ref``."""
    lbt, slb, blb = _bound(lb, n, dt, dev)
    ubt, sub, bub = _bound(ub, n, dt, dev)
    for name, t in (("lb", lbt), ("ub", ubt)):
        if t is not None and t.shape[-1] != n:
            raise ValueError(f"{name}: last dimension {t.shape[-1]} != n = {n}")
    _batch_of((1, batch), *insts, (slb, blb), (sub, bub))
    if status is not None:
        if status.dtype != torch.int32 or tuple(status.shape) != status_shape or status.device != dev:
            what = "(batch,)" if len(status_shape) == 1 else "(T, batch)"
            raise ValueError(f"status must be the forward's {what} int32 device tensor")
        status = status.contiguous()

    def shared(g, stride, ref=None):
        if g is None or stride != 0:
            return g
        g = g.sum(0)
        return g if ref is None else g.reshape(ref.shape)

    return lbt, slb, ubt, sub, status, shared


def solve_box_vjp(H, z, lb, ub, gz, *, status=None, need_H: bool = True) -> dict:
    """Adjoint of ``solve_box`` at its optimum ``z`` (include/mpcqp.h
    ``mpcqp_solve_box_vjp``): from ``gz = dL/dz`` (b, n) the gradients

    * ``gf``  = d, with d_F = -H_FF^-1 gz_F on the free rows and 0 on the rows
      at a bound (compared exactly);
    * ``glb`` / ``gub`` = nu = gz_A + H_AF d_F on the side the row sits at;
    * ``gH`` (packed lower, only with ``need_H``; else None): d z' folded onto
      the packed entries, (i, j<i) = d_i z_j + d_j z_i, (i, i) = d_i z_i;
    * ``vstatus`` (b,) int32: a bare status code; where it is not OPTIMAL every
      gradient of the instance is exactly zero.

    H, lb, ub as in ``solve_box`` (shared without a batch dimension, scalar or
    None bounds); ``status`` is the forward's status (None = all optimal).  The
    gradient of a shared H, lb or ub is summed over the batch and has the
    shared shape.  A row at a bound with a zero multiplier counts as active
    (one-sided derivative).  n <= 32."""
    dt, dev = z.dtype, z.device
    z = _dev(z, dt, dev)
    gz = _dev(gz, dt, dev)
    H = _dev(H, dt, dev)
    if z.ndim != 2 or gz.shape != z.shape:
        raise ValueError(f"z and gz must both be (batch, n), got {tuple(z.shape)} and {tuple(gz.shape)}")
    batch, n = int(z.shape[0]), int(z.shape[1])
    if H.shape[-1] != n * (n + 1) // 2:
        raise ValueError(f"H must be packed lower with {n * (n + 1) // 2} entries, got {tuple(H.shape)}")
    sH, bH = _inst(H, 1, "H")
    lbt, slb, ubt, sub, status, shared = _vjp_common(lb, ub, n, dt, dev, batch, [(sH, bH)],
                                                     status, (batch,))
    gf, glb, gub, gH, vstatus = _alloc(
        {"gf": ((batch, n), dt), "glb": ((batch, n), dt), "gub": ((batch, n), dt),
         "gH": ((batch, n * (n + 1) // 2), dt) if need_H else None,
         "vstatus": ((batch,), torch.int32)}, dev)
    rc = _lib().mpcqp_solve_box_vjp(_code(dt), batch, n, _ptr(H), sH, _ptr(z), _ptr(lbt), slb,
                                    _ptr(ubt), sub, _ptr(status), _ptr(gz), _ptr(gf), _ptr(glb),
                                    _ptr(gub), _ptr(gH), _ptr(vstatus), _stream())
    nat.check(rc, "mpcqp_solve_box_vjp")
    return {"gf": gf, "glb": shared(glb, slb), "gub": shared(gub, sub), "gH": shared(gH, sH),
            "vstatus": vstatus}


LOOP_VJP_OUTPUTS = ("gx0", "gH", "gF", "gA", "gB", "glb", "gub", "gg", "gw")


def mpc_box_loop_vjp(H, F, A, B, lb, ub, xs, zs, gxs=None, gus=None, gzs=None, *, status=None,
                     need=LOOP_VJP_OUTPUTS) -> dict:
    """Adjoint of ``mpc_box_loop`` over the whole episode, one launch
    (include/mpcqp.h ``mpcqp_mpc_box_loop_vjp``).  ``xs`` (T+1, b, nx), ``zs``
    (T, b, n) and ``status`` (T, b; None = every step optimal) are the
    forward's outputs; H (packed), F, A, B, lb, ub its inputs (shared without a
    batch dimension, or per instance; a leading dimension of 1 counts as
    shared).  ``gxs`` (T+1, b, nx), ``gus`` (T, b, nu), ``gzs`` (T, b, n) are
    dL/dxs, dL/dus, dL/dzs; None means zero.  Returns a dict with the entries of
    ``need`` (the others None) out of

    * ``gx0`` (b, nx); ``gg`` (T, b, n) = dL/dg_t; ``gw`` (T, b, nx) = dL/dw_t;
    * ``gH`` (packed, folded as in ``solve_box_vjp``), ``gF``, ``gA``, ``gB``,
      ``glb``, ``gub``: in the shape of the input, summed over the batch where
      the input is shared;

    and ``vstatus`` (b,) int32, a bare status code: where it is not OPTIMAL
    every gradient of the instance is exactly zero.  Limits of the loop: nx <=
    4, nu <= 2, n <= 32."""
    dt, dev = xs.dtype, xs.device
    xs, zs = _dev(xs, dt, dev), _dev(zs, dt, dev)
    H, F, A, B = _dev(H, dt, dev), _dev(F, dt, dev), _dev(A, dt, dev), _dev(B, dt, dev)
    if xs.ndim != 3 or zs.ndim != 3 or xs.shape[0] != zs.shape[0] + 1 or xs.shape[1] != zs.shape[1]:
        raise ValueError(f"xs must be (T+1, b, nx) and zs (T, b, n), got {tuple(xs.shape)} and "
                         f"{tuple(zs.shape)}")
    T, batch, n = (int(v) for v in zs.shape)
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    if xs.shape[2] != nx or n % nu or H.shape[-1] != n * (n + 1) // 2 \
            or tuple(F.shape[-2:]) != (n, nx) or tuple(A.shape[-2:]) != (nx, nx):
        raise ValueError(f"inconsistent shapes: H {tuple(H.shape)}, F {tuple(F.shape)}, A "
                         f"{tuple(A.shape)}, B {tuple(B.shape)}, xs {tuple(xs.shape)}, zs "
                         f"{tuple(zs.shape)}")
    unknown = set(need) - set(LOOP_VJP_OUTPUTS)
    if unknown:
        raise ValueError(f"need: unknown outputs {sorted(unknown)}")

    # a leading 1 of H, F, A or B is shared, unless the batch itself is 1
    (sH, bH), (sF, bF), (sA, bA), (sB, bB) = (
        _inst_one(t, nd, name, batch > 1) for t, nd, name in ((H, 1, "H"), (F, 2, "F"),
                                                              (A, 2, "A"), (B, 2, "B")))
    lbt, slb, ubt, sub, status, shared = _vjp_common(
        lb, ub, n, dt, dev, batch, [(sH, bH), (sF, bF), (sA, bA), (sB, bB)], status, (T, batch))
    ups = {}
    for name, t, shp in (("gxs", gxs, (T + 1, batch, nx)), ("gus", gus, (T, batch, nu)),
                         ("gzs", gzs, (T, batch, n))):
        t = _dev(t, dt, dev)
        if t is not None and tuple(t.shape) != shp:
            raise ValueError(f"{name} must be {shp}, got {tuple(t.shape)}")
        ups[name] = t
    shapes = dict(gx0=(batch, nx), gH=(batch, n * (n + 1) // 2), gF=(batch, n, nx),
                  gA=(batch, nx, nx), gB=(batch, nx, nu), glb=(batch, n), gub=(batch, n),
                  gg=(T, batch, n), gw=(T, batch, nx))
    spec = {k: (shapes[k], dt) if k in need else None for k in LOOP_VJP_OUTPUTS}
    o = _alloc({**spec, "vstatus": ((batch,), torch.int32)}, dev, keyed=True)
    rc = _lib().mpcqp_mpc_box_loop_vjp(
        _code(dt), batch, nx, nu, n // nu, T, _ptr(H), sH, _ptr(F), sF, _ptr(A), sA, _ptr(B), sB,
        _ptr(lbt), slb, _ptr(ubt), sub, _ptr(xs), _ptr(zs), _ptr(status), _ptr(ups["gxs"]),
        _ptr(ups["gus"]), _ptr(ups["gzs"]), *(_ptr(o[k]) for k in LOOP_VJP_OUTPUTS),
        _ptr(o["vstatus"]), _stream())
    nat.check(rc, "mpcqp_mpc_box_loop_vjp")
    for k, s, ref in (("gH", sH, H), ("gF", sF, F), ("gA", sA, A), ("gB", sB, B),
                      ("glb", slb, None), ("gub", sub, None)):
        o[k] = shared(o[k], s, ref)
    return o


# ------------------------------------------------------------- polytope QP
def _poly_box(v, n, dt, dev, name):
    """lbz / ubz of the polytope QP: shared by the batch, a scalar or (n,)."""
    t = _bound(v, n, dt, dev)[0]
    if t is not None and tuple(t.shape) != (n,):
        raise ValueError(f"{name} must be a scalar or ({n},), got {tuple(t.shape)}")
    return t


def _poly_vec(t, width, name):
    """(stride, batch) of a (width,) shared or (batch, width) per-instance operand."""
    if t is None:
        return 0, None
    shape = t.shape
    if len(shape) not in (1, 2) or shape[-1] != width:
        raise ValueError(f"{name} must be ({width},) or (batch, {width}), got {tuple(shape)}")
    return (width, int(shape[0])) if len(shape) == 2 else (0, None)


def _poly_rows(hl, hu, m):
    """(stride, batch) of the row bounds: both shared or both per instance."""
    _, _, sh, bl, bu = _row_pair(
        hl, hu, "raise", lambda t, k: (t, *_poly_vec(t, m, ("hl", "hu")[k])),
        "hl and hu must both be shared or both per instance, got {lo} and {hi}")
    if bl is not None and bu is not None and bl != bu:
        raise ValueError(f"hl and hu have different batch sizes {bl} and {bu}")
    return sh, bl if bl is not None else bu


def _poly_out(out, batch, n, mt, dt, dev):
    """z, y, status of a polytope solve: allocated, or the checked ``out``
    triple (contiguous, of dtype ``dt`` on the operands' device ``dev``)."""
    return _alloc({"z": ((batch, n), dt), "y": ((batch, mt), dt),
                   "status": ((batch,), torch.int32)}, dev, out, check=True)


def solve_poly(H, f, G=None, hl=None, hu=None, lbz=None, ubz=None, *, max_iter: int = 0,
               tol: float = 0.0, out: tuple | None = None):
    """Batched  min 1/2 z'Hz + f'z  s.t.  hl <= G z <= hu,  lbz <= z <= ubz.

    H (packed, shared) and G (m, n) shared; f (n,) | (b, n); hl, hu (m,) |
    (b, m), both shared or both per instance; lbz, ubz a scalar or (n,).
    Returns (z, y, status); y are the multipliers of the rows [G; I]
    (``out``: a preallocated contiguous triple to write them to).  Malformed
    operands raise ValueError before anything is launched.
    """
    dt, dev = f.dtype, f.device
    f = _dev(f, dt, dev)
    H = _dev(H, dt, dev)
    if f.ndim not in (1, 2):
        raise ValueError(f"f must be (n,) or (batch, n), got {tuple(f.shape)}")
    n = int(f.shape[-1])
    if H.ndim != 1:
        raise ValueError("solve_poly: H must be shared (packed, 1-D)")
    if H.shape[0] != n * (n + 1) // 2:
        raise ValueError(f"H must be packed lower with {n * (n + 1) // 2} entries for f of width "
                         f"{n}, got {tuple(H.shape)}")
    G = _dev(G, dt, dev)
    if G is not None and (G.ndim != 2 or G.shape[1] != n):
        raise ValueError(f"G must be (m, {n}), got {tuple(G.shape)}")
    m = 0 if G is None else int(G.shape[0])
    sf, bf = _poly_vec(f, n, "f")
    hl = _dev(hl, dt, dev)
    hu = _dev(hu, dt, dev)
    sh, bh = _poly_rows(hl, hu, m)
    lbz_t = _poly_box(lbz, n, dt, dev, "lbz")
    ubz_t = _poly_box(ubz, n, dt, dev, "ubz")
    nbox = 1 if (lbz_t is not None or ubz_t is not None) else 0
    mt = m + (n if nbox else 0)
    batch = _batch_of((sf, bf), (sh, bh))
    z, y, status = _poly_out(out, batch, n, mt, dt, dev)
    lib = _lib()
    wsb = int(lib.mpcqp_solve_poly_workspace(_code(dt), batch, n, m, nbox))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    rc = lib.mpcqp_solve_poly(_code(dt), batch, n, m, _ptr(H), _ptr(f), sf, _ptr(G), _ptr(hl),
                              _ptr(hu), sh, _ptr(lbz_t), _ptr(ubz_t), _ptr(z), _ptr(y),
                              _ptr(status), int(max_iter), float(tol), _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_solve_poly")
    return z, y, status


class PolyQP:
    """Shared-structure polytope QP for the receding-horizon loop
    (include/mpcqp.h ``mpcqp_poly_setup`` / ``mpcqp_poly_solve``):

        min 1/2 z'Hz + (F x0 + f)'z   s.t.  hl <= G z <= hu,  lbz <= z <= ubz

    H (packed, n(n+1)/2), G (m, n) and F (n, nx) are fixed at construction
    (the factors are formed once on device); ``solve`` takes a batch of x0
    and/or extra gradients f and per-instance or shared row bounds.
    """

    def __init__(self, H, G=None, F=None, lbz=None, ubz=None, *, dtype=None, device=None):
        dt = dtype or H.dtype
        dev = device or H.device
        self.dtype, self.device = dt, dev
        self.H = _dev(H, dt, dev)
        self.n = n = isqrt_packed(int(self.H.shape[-1]))
        if self.H.ndim != 1:
            raise ValueError("PolyQP: H must be shared (packed, 1-D)")
        self.G = _dev(G, dt, dev)
        if G is not None and (self.G.ndim != 2 or self.G.shape[1] != n):
            raise ValueError(f"G must be (m, {n}), got {tuple(self.G.shape)}")
        self.m = 0 if G is None else int(self.G.shape[0])
        self.F = _dev(F, dt, dev)
        if F is not None and (self.F.ndim != 2 or self.F.shape[0] != n):
            raise ValueError(f"F must be ({n}, nx), got {tuple(self.F.shape)}")
        self.nx = 0 if F is None else int(self.F.shape[-1])
        self.lbz = _poly_box(lbz, n, dt, dev, "lbz")
        self.ubz = _poly_box(ubz, n, dt, dev, "ubz")
        self.nbox = 1 if (self.lbz is not None or self.ubz is not None) else 0
        self.mt = self.m + (n if self.nbox else 0)
        lib = _lib()
        wsb = int(lib.mpcqp_poly_workspace(_code(dt), n, self.m, self.nbox, self.nx))
        self.ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        rc = lib.mpcqp_poly_setup(_code(dt), n, self.m, self.nbox, self.nx, _ptr(self.H),
                                  _ptr(self.G), _ptr(self.F), _ptr(self.ws), wsb, _stream())
        nat.check(rc, "mpcqp_poly_setup")

    def solve(self, x0=None, f=None, hl=None, hu=None, *, max_iter: int = 0, tol: float = 0.0,
              out: tuple | None = None):
        """x0 (nx,) | (b, nx), f (n,) | (b, n), hl and hu (m,) | (b, m), both
        shared or both per instance; ``out`` a preallocated (z, y, status).
        Returns (z (b, n), y (b, m_total), status (b,))."""
        dt, dev, n = self.dtype, self.device, self.n
        x0, f = _dev(x0, dt, dev), _dev(f, dt, dev)
        hl, hu = _dev(hl, dt, dev), _dev(hu, dt, dev)
        if x0 is not None and self.nx == 0:
            raise ValueError("x0 given, but this PolyQP has no x0 -> gradient map F")
        sX, bX = _poly_vec(x0, self.nx, "x0")
        sf, bf = _poly_vec(f, n, "f")
        sh, bh = _poly_rows(hl, hu, self.m)
        batch = _batch_of((sX, bX), (sf, bf), (sh, bh))
        # self.device may lack an index ("cuda"); the workspace's has one, as out's do
        z, y, status = _poly_out(out, batch, n, self.mt, dt, self.ws.device)
        rc = _lib().mpcqp_poly_solve(_code(dt), batch, n, self.m, self.nbox, self.nx,
                                     _ptr(self.ws), _ptr(x0), sX, _ptr(f), sf, _ptr(hl), _ptr(hu),
                                     sh, _ptr(self.lbz), _ptr(self.ubz), _ptr(z), _ptr(y),
                                     _ptr(status), int(max_iter), float(tol), _stream())
        nat.check(rc, "mpcqp_poly_solve")
        return z, y, status

    def affine_scratch_bytes(self, batch: int, steps: int, g_shared: bool) -> int:
        """Bytes of scratch ``loop(g=...)`` needs (``mpcqp_mpc_poly_loop_affine_workspace``)."""
        return int(_lib().mpcqp_mpc_poly_loop_affine_workspace(
            _code(self.dtype), int(batch), self.n, self.m, self.nbox, int(steps),
            1 if g_shared else 0))

    def loop(self, A, B, x0, steps: int, hl=None, hu=None, E=None, w=None, *,
             plans: bool = False, multipliers: bool = False, cold: bool = False,
             max_iter: int = 0, tol: float = 0.0, out: dict | None = None,
             soft: tuple | None = None, slacks: bool = False, g=None, e=None) -> dict:
        """The receding-horizon loop on this object's factors, ``steps`` steps
        in one launch (include/mpcqp.h ``mpcqp_mpc_poly_loop``): per step
        z_t = argmin 1/2 z'Hz + (F x_t)'z over hl - E x_t <= G z <= hu - E x_t,
        lbz <= z <= ubz; u_t = z_t[:nu]; x_{t+1} = A x_t + B u_t (+ w_t).

        A (nx, nx), B (nx, nu): the simulated plant (shared); x0 (b, nx); hl, hu
        (m,) | (b, m); E (m, nx) or None; w (steps, b, nx) or None.  Each step
        starts from the previous step's active set unless ``cold``.  Returns
        xs (steps+1, b, nx), us (steps, b, nu), status (steps, b), with
        ``plans`` zs (steps, b, n), with ``multipliers`` ys (steps, b, m_total).

        ``soft=(rho, sigma)`` (scalars or (m,), shared by the batch) softens
        the rows of G with the exact penalty rho_i eps_i + 1/2 sigma_i eps_i^2
        on a slack eps_i >= 0 shared by the row's two sides
        (``mpcqp_mpc_poly_loop_soft``); rho_i = inf keeps row i hard, the
        input box always is.  A step that ends with a slack > 0 carries
        ``STATUS_SOFTENED`` in its status word; with ``slacks`` eps (steps, b,
        m) is returned too.

        ``g`` ((steps, n) shared by the batch, or (steps, b, n)) is a per-step
        linear term: the step's gradient is F x_t + g_t (``tracking_terms``
        builds it from a reference trajectory); ``e`` ((steps, m) or (steps,
        b, m)) moves the bounds of the rows of G by -e_t.  With either the
        call goes to ``mpcqp_mpc_poly_loop_affine``; its scratch (the products
        -Hinv g, -Ut g of all steps) is allocated here or taken from
        ``out["scratch"]`` (uint8, at least ``affine_scratch_bytes``)."""
        dt, dev, n, m, nx = self.dtype, self.device, self.n, self.m, self.nx
        if nx == 0:
            raise ValueError("PolyQP.loop needs the x0 -> gradient map F at construction")
        A, B, x0 = _dev(A, dt, dev), _dev(B, dt, dev), _dev(x0, dt, dev)
        if tuple(A.shape) != (nx, nx):
            raise ValueError(f"A must be ({nx}, {nx}), got {tuple(A.shape)}")
        if B.ndim != 2 or B.shape[0] != nx:
            raise ValueError(f"B must be ({nx}, nu), got {tuple(B.shape)}")
        nu = int(B.shape[1])
        if not 1 <= nu <= min(16, n):
            raise ValueError(f"nu={nu} outside [1, min(16, n={n})]")
        if x0.ndim != 2 or x0.shape[1] != nx:
            raise ValueError(f"x0 must be (batch, {nx}), got {tuple(x0.shape)}")
        batch, T = int(x0.shape[0]), int(steps)
        if T < 0:
            raise ValueError(f"steps={T} < 0")
        hl, hu = _dev(hl, dt, dev), _dev(hu, dt, dev)

        def side(h, k):
            if h is None:
                return None, 0, None
            if h.shape[-1] != m or h.ndim not in (1, 2) or (h.ndim == 2 and h.shape[0] != batch):
                raise ValueError(f"{('hl', 'hu')[k]} must be ({m},) or ({batch}, {m}), got "
                                 f"{tuple(h.shape)}")
            return (h, m, batch) if h.ndim == 2 else (h, 0, None)

        sh = _row_pair(hl, hu, "raise", side,
                       "hl and hu must both be shared or both per instance")[2]
        E = _dev(E, dt, dev)
        if E is not None and tuple(E.shape) != (m, nx):
            raise ValueError(f"E must be ({m}, {nx}), got {tuple(E.shape)}")
        w = _dev(w, dt, dev)
        if w is not None and tuple(w.shape) != (T, batch, nx):
            raise ValueError(f"w must be ({T}, {batch}, {nx}), got {tuple(w.shape)}")
        g, e = _dev(g, dt, dev), _dev(e, dt, dev)
        for name, v, width in (("g", g, n), ("e", e, m)):
            if v is not None and tuple(v.shape) not in ((T, width), (T, batch, width)):
                raise ValueError(f"{name} must be ({T}, {width}) or ({T}, {batch}, {width}), "
                                 f"got {tuple(v.shape)}")
        rho = sigma = None
        if soft is not None:
            if not isinstance(soft, (tuple, list)) or len(soft) != 2:
                raise ValueError("soft must be a pair (rho, sigma)")
            pen = []
            for name, v in zip(("rho", "sigma"), soft):
                v = torch.as_tensor(v, dtype=dt, device=dev)
                if v.ndim == 0:
                    v = v.expand(m)
                if tuple(v.shape) != (m,):
                    raise ValueError(f"soft {name} must be a scalar or ({m},), got {tuple(v.shape)}")
                pen.append(v.contiguous())
            rho, sigma = pen
        elif slacks:
            raise ValueError("slacks=True needs soft=(rho, sigma)")
        o = dict(out or {})
        scratch, sb = o.pop("scratch", None), 0
        if g is not None:
            sb = self.affine_scratch_bytes(batch, T, g.ndim == 2)
            if scratch is None:
                scratch = torch.empty((sb,), dtype=torch.uint8, device=dev)
            elif (scratch.dtype != torch.uint8 or scratch.ndim != 1 or scratch.numel() < sb
                  or scratch.device != x0.device):
                raise ValueError(f"out['scratch'] must be a uint8 tensor of at least {sb} bytes "
                                 f"on {dev}")
            else:
                sb = int(scratch.numel())
        spec = dict(xs=((T + 1, batch, nx), dt), us=((T, batch, nu), dt),
                    status=((T, batch), torch.int32))
        if slacks:
            spec["eps"] = ((T, batch, m), dt)
        if plans:
            spec["zs"] = ((T, batch, n), dt)
        if multipliers:
            spec["ys"] = ((T, batch, self.mt), dt)
        o = _alloc(spec, dev, o, keyed=True, check=True)
        head = (_code(dt), batch, n, m, self.nbox, nx, nu, T, nat.LOOP_COLD if cold else 0,
                _ptr(self.ws), _ptr(E), _ptr(A), _ptr(B), _ptr(x0), nx, _ptr(hl), _ptr(hu), sh,
                _ptr(self.lbz), _ptr(self.ubz), _ptr(w))
        outs = (_ptr(o["xs"]), _ptr(o["us"]), _ptr(o.get("zs")), _ptr(o.get("ys")))
        tail = (_ptr(o["status"]), int(max_iter), float(tol), _stream())
        eps = _ptr(o.get("eps"))
        if g is not None or e is not None:
            if rho is None or m == 0:
                rho = sigma = None
            rc = _lib().mpcqp_mpc_poly_loop_affine(
                *head, _ptr(rho), _ptr(sigma), _ptr(g), 0 if g is None or g.ndim == 2 else n,
                _ptr(e), 0 if e is None or e.ndim == 2 else m, _ptr(scratch), sb, *outs, eps, *tail)
            nat.check(rc, "mpcqp_mpc_poly_loop_affine")
            if scratch is not None:
                o["scratch"] = scratch
            return o
        if rho is not None and m > 0:
            rc = _lib().mpcqp_mpc_poly_loop_soft(*head, _ptr(rho), _ptr(sigma), *outs, eps, *tail)
            nat.check(rc, "mpcqp_mpc_poly_loop_soft")
            return o
        rc = _lib().mpcqp_mpc_poly_loop(*head, *outs, *tail)
        nat.check(rc, "mpcqp_mpc_poly_loop")
        return o


def tracking_terms(cd, Q, R, Qf, N: int, T: int, x_ref=None, u_ref=None):
    """The per-step linear term g of ``PolyQP.loop`` for the tracking cost
    sum_k (x_k - r_{t+k})'Q(x_k - r_{t+k}) + (u_k - ubar_{t+k})'R(u_k - ubar_{t+k})
    (terminal weight Qf) of an MPC condensed as ``cd`` (a dict with Gam, (N*nx,
    N*nu), or (b, N*nx, N*nu) from per-instance plants):  g_t = -Gam' Qhat rbar_t - Rhat ubar_t  with Qhat = blkdiag(Q, ..,
    Q, Qf), Rhat = blkdiag(R, .., R), rbar_t = x_ref[t+1 : t+N+1], ubar_t =
    u_ref[t : t+N], both references indexed by absolute time: x_ref (nx,)
    (a setpoint), (T+N+1, nx) or (b, T+N+1, nx); u_ref (nu,), (T+N, nu) or (b,
    T+N, nu).  Returns g (T, n), or (T, b, n) when a reference or Gam is per
    instance.  Plain tensor algebra on the device of ``cd`` (CPU tensors work
    too)."""
    Gam = cd["Gam"]
    if Gam.ndim not in (2, 3):
        raise ValueError(f"Gam must be (N*nx, n) or (b, N*nx, n), got {tuple(Gam.shape)}")
    dt, dev = Gam.dtype, Gam.device
    N, T = int(N), int(T)
    n = int(Gam.shape[-1])
    nx, nu = int(Gam.shape[-2]) // N, n // N
    as_t = lambda v: torch.as_tensor(v, dtype=dt, device=dev)  # noqa: E731
    if x_ref is None and u_ref is None:
        raise ValueError("tracking_terms needs x_ref or u_ref")

    def windows(ref, width, length, first, name):
        """(T, N*width) or (b, T, N*width): the N-step windows from ``first``"""
        r = as_t(ref)
        if tuple(r.shape) == (width,):
            r = r.expand(length, width)
        if r.ndim not in (2, 3) or tuple(r.shape[-2:]) != (length, width):
            raise ValueError(f"{name} must be ({width},), ({length}, {width}) or (b, {length}, "
                             f"{width}), got {tuple(r.shape)}")
        win = r[..., first:, :].unfold(-2, N, 1)[..., :T, :, :]     # (.., T, width, N)
        return win.transpose(-1, -2).reshape(*r.shape[:-2], T, N * width)

    parts, mats = [], []
    if x_ref is not None:
        Qhat = torch.block_diag(*([as_t(Q).reshape(nx, nx)] * (N - 1) + [as_t(Qf).reshape(nx, nx)]))
        parts.append(windows(x_ref, nx, T + N + 1, 1, "x_ref"))
        mats.append(Qhat.T @ Gam)                                    # (N*nx, n)
    if u_ref is not None:
        parts.append(windows(u_ref, nu, T + N, 0, "u_ref"))
        mats.append(torch.block_diag(*([as_t(R).reshape(nu, nu)] * N)).T)
    if len(parts) == 2 and parts[0].ndim != parts[1].ndim:
        b = max(parts, key=lambda v: v.ndim).shape[0]
        parts = [v if v.ndim == 3 else v.expand(b, *v.shape) for v in parts]
    if len(parts) == 2 and parts[0].shape[:-1] != parts[1].shape[:-1]:
        raise ValueError("x_ref and u_ref have different batch sizes")
    if Gam.ndim == 3:
        # per-instance plants: the state part is a batched product, (b, T, n)
        if parts[0].ndim == 3 and parts[0].shape[0] != Gam.shape[0]:
            raise ValueError(f"the references have batch {parts[0].shape[0]}, Gam {Gam.shape[0]}")
        g = torch.zeros((Gam.shape[0], T, n), dtype=dt, device=dev)
        for v, mat in zip(parts, mats):
            g = g - v @ mat
        return g.transpose(0, 1).contiguous()
    g = -(torch.cat(parts, dim=-1) @ torch.cat(mats, dim=0))
    return g.transpose(0, 1).contiguous() if g.ndim == 3 else g.contiguous()


def _stage_bound(v, width: int, N: int, dt, dev, name: str):
    """A stage bound (scalar or (width,)) tiled over the N stages, or (N * width,)
    as it is; None stays None."""
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=dt, device=dev)
    if t.ndim == 0 or tuple(t.shape) == (width,):
        return t.expand(width).repeat(N)
    if tuple(t.shape) == (N * width,):
        return t
    raise ValueError(f"{name}: expected a scalar, ({width},) or ({N * width},), "
                     f"got {tuple(t.shape)}")


def mpc_poly_loop(A, B, Q, R, Qf, N: int, x0, xlo=None, xhi=None, lb=None, ub=None,
                  steps: int = 1, *, plant=None, w=None, plans: bool = False,
                  multipliers: bool = False, cold: bool = False, max_iter: int = 0,
                  tol: float = 0.0, soft: tuple | None = None, slacks: bool = False,
                  x_ref=None, u_ref=None) -> dict:
    """The receding-horizon loop of the linear MPC with a state box on
    x_1..x_N and an input box (sessions 2 and 3, session_2/problem.py:4-33), on
    the device in one launch.  The shared model (A, B) is condensed once (H, F,
    Gam, Phi); the state box becomes the rows xlo - Phi x_t <= Gam z <= xhi -
    Phi x_t of a ``PolyQP`` (G = Gam, E = Phi), lb/ub (scalar, (nu,) or
    (N*nu,)) its input box, and ``PolyQP.loop`` runs the episode.
    ``plant=(A_p, B_p)`` simulates another plant than the controller's model.
    x0 (b, nx); xlo/xhi (nx,) or None.  ``soft=(rho, sigma)`` softens the
    state box (``PolyQP.loop``): each a scalar, (nx,) per state component or
    (N*nx,) per row; ``slacks`` returns eps (steps, b, N*nx).  Returns the
    dict of ``PolyQP.loop`` plus ``condensed`` (H, F, Gam, Phi of the model,
    unbatched).  ``x_ref`` / ``u_ref`` (shapes of ``tracking_terms``) make
    the cost track a reference trajectory with preview instead of the origin;
    the state and input boxes stay boxes on x and u."""
    dt, dev = _dt_dev(A)
    A, B = _dev(A, dt, dev), _dev(B, dt, dev)
    if A.ndim != 2 or B.ndim != 2:
        raise ValueError("mpc_poly_loop: the model (A, B) is shared by the batch")
    nx, nu = int(B.shape[0]), int(B.shape[1])
    n = N * nu
    cd = condense(A, B, Q, R, Qf, N, outputs=("H", "F", "Gam", "Phi"))
    cd = {k: v[0] for k, v in cd.items()}

    hl, hu, lbz, ubz = (_stage_bound(v, width, N, dt, dev, name) for v, width, name in (
        (xlo, nx, "xlo"), (xhi, nx, "xhi"), (lb, nu, "lb"), (ub, nu, "ub")))
    rows = hl is not None or hu is not None
    qp = PolyQP(cd["H"], cd["Gam"] if rows else None, cd["F"], lbz, ubz)
    Ap, Bp = (A, B) if plant is None else plant
    if soft is not None:
        if not isinstance(soft, (tuple, list)) or len(soft) != 2:
            raise ValueError("soft must be a pair (rho, sigma)")
        if not rows:
            raise ValueError("soft needs a state box (xlo or xhi)")
        soft = (_stage_bound(soft[0], nx, N, dt, dev, "soft rho"),
                _stage_bound(soft[1], nx, N, dt, dev, "soft sigma"))
    g = None
    if x_ref is not None or u_ref is not None:
        g = tracking_terms(cd, _dev(Q, dt, dev), _dev(R, dt, dev), _dev(Qf, dt, dev), N, steps,
                           x_ref, u_ref)
    o = qp.loop(Ap, Bp, x0, steps, hl, hu, cd["Phi"] if rows else None, w, plans=plans,
                multipliers=multipliers, cold=cold, max_iter=max_iter, tol=tol, soft=soft,
                slacks=slacks, g=g)
    o["condensed"] = cd
    return o


# ------------------------------------------ general QP, per-instance rows
def solve_qp(H, f, G=None, hl=None, hu=None, lb=None, ub=None, *, max_iter: int = 0,
             tol: float = 0.0, out: tuple | None = None, presweep: bool = True,
             ws: torch.Tensor | None = None):
    """Batched  min 1/2 z'Hz + f'z  s.t.  lb <= z <= ub,  hl <= G z <= hu.

    Every operand may be per instance (leading batch dim) or shared: H packed
    lower (n(n+1)/2), G (m, n), hl/hu (m), lb/ub (n).  n + m <= 192.
    One instance per workgroup (libmpcqp ``mpcqp_solve_qp``); fp32 with
    64 < n + m runs the z sweep first as its own MFMA kernel
    (``mpcqp_solve_qp_ws``) unless ``presweep=False``.
    Returns (z, y, status); y (batch, m) are the row multipliers
    (y > 0 at the upper bound, y < 0 at the lower bound).
    ``ws``: optional caller-owned scratch (``workspace_bytes(dtype, batch, n, m)``).
    """
    dt, dev = f.dtype, f.device
    f = _dev(f, dt, dev)
    H = _dev(H, dt, dev)
    n = int(f.shape[-1])
    if H.shape[-1] != n * (n + 1) // 2:
        raise ValueError(f"H must be packed lower with {n * (n + 1) // 2} entries, got {tuple(H.shape)}")
    sH, bH = _inst(H, 1, "H")
    sf, bf = _inst(f, 1, "f")
    m = 0 if G is None else int(G.shape[-2])
    G = _dev(G, dt, dev)
    sG, bG = (0, None) if G is None else _inst(G, 2, "G")
    hl = _dev(hl, dt, dev)
    hu = _dev(hu, dt, dev)
    _, _, sh, bhl, bhu = _row_pair(hl, hu, "equal", lambda t, _: (t, *_inst(t, 1, "h")),
                                   "hl and hu must have the same shape")
    lbt, slb, blb = _bound(lb, n, dt, dev)
    ubt, sub, bub = _bound(ub, n, dt, dev)
    batch = _batch_of((sH, bH), (sf, bf), (sG, bG), (sh, bhl), (sh, bhu), (slb, blb), (sub, bub))
    z, y, status = _alloc({"z": ((batch, n), dt), "y": ((batch, m), dt) if m else None,
                           "status": ((batch,), torch.int32)}, dev, out)
    lib = _lib()
    wsb = int(lib.mpcqp_solve_qp_workspace(_code(dt), batch, n, m)) if presweep else 0
    ws = _workspace(wsb, dev, ws)
    rc = lib.mpcqp_solve_qp_ws(_code(dt), batch, n, m, _ptr(H), sH, _ptr(f), sf, _ptr(G), sG,
                               _ptr(hl), _ptr(hu), sh, _ptr(lbt), slb, _ptr(ubt), sub, _ptr(z),
                               _ptr(y), _ptr(status), int(max_iter), float(tol), _ptr(ws), wsb,
                               _stream())
    nat.check(rc, "mpcqp_solve_qp_ws")
    return z, y, status


def sweep(H, G=None, *, full: bool = False):
    """Batched M = SWEEP_z([[H, G'], [G, 0]]) (libmpcqp ``mpcqp_sweep``, fp32,
    MFMA): returns (M, status) with M = [[-H^-1, H^-1 G'], [G H^-1, -G H^-1 G']]
    over n + m per instance, packed lower, or dense (n+m, n+m) if ``full``."""
    dt, dev = H.dtype, H.device
    H = _dev(H, dt, dev)
    nH = int(H.shape[-1])
    n = isqrt_packed(nH)
    sH, bH = _inst(H, 1, "H")
    m = 0 if G is None else int(G.shape[-2])
    G = _dev(G, dt, dev)
    sG, bG = (0, None) if G is None else _inst(G, 2, "G")
    batch = _batch_of((sH, bH), (sG, bG))
    nt = n + m
    shape = (batch, nt, nt) if full else (batch, nt * (nt + 1) // 2)
    M = torch.empty(shape, dtype=dt, device=dev)
    status = torch.empty((batch,), dtype=torch.int32, device=dev)
    rc = _lib().mpcqp_sweep(_code(dt), batch, n, m, _ptr(H), sH, _ptr(G), sG, _ptr(M),
                            int(bool(full)), _ptr(status), _stream())
    nat.check(rc, "mpcqp_sweep")
    return M, status


# ---------------------------------------------------------------- Riccati
def riccati(A, B, Q, R, Pf, N: int):
    """Batched FHC.ricatti_recursion: returns P (b,N+1,nx,nx), K (b,N,nu,nx)."""
    dt = A.dtype
    dev = A.device
    A, B, Q, R, Pf = (_dev(v, dt, dev) for v in (A, B, Q, R, Pf))
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    R = _weight_r(R, nu)
    sA, bA = _inst(A, 2, "A")
    sB, bB = _inst(B, 2, "B")
    sQ, bQ = _inst(Q, 2, "Q")
    sR, bR = _inst(R, 2, "R")
    sP, bP = _inst(Pf, 2, "Pf")
    batch = _batch_of((sA, bA), (sB, bB), (sQ, bQ), (sR, bR), (sP, bP))
    P = torch.empty((batch, N + 1, nx, nx), dtype=dt, device=dev)
    K = torch.empty((batch, N, nu, nx), dtype=dt, device=dev)
    rc = _lib().mpcqp_riccati(_code(dt), batch, nx, nu, N, _ptr(A), sA, _ptr(B), sB, _ptr(Q), sQ,
                              _ptr(R), sR, _ptr(Pf), sP, _ptr(P), _ptr(K), _stream())
    nat.check(rc, "mpcqp_riccati")
    return P, K


# ------------------------------------------------------------------ gemv
def gemv(M, x, alpha: float = 1.0, beta: float = 0.0, y=None):
    """Batched y = alpha M x + beta y; M (r,c) shared or (b,r,c); x (c,) or (b,c)."""
    dt, dev = x.dtype, x.device
    M, x = _dev(M, dt, dev), _dev(x, dt, dev)
    rows, cols = int(M.shape[-2]), int(M.shape[-1])
    sM, bM = _inst(M, 2, "M")
    sX, bX = _inst(x, 1, "x")
    batch = _batch_of((sM, bM), (sX, bX))
    if y is None:
        y = torch.zeros((batch, rows), dtype=dt, device=dev)
    rc = _lib().mpcqp_gemv(_code(dt), batch, rows, cols, float(alpha), _ptr(M), sM, _ptr(x), sX,
                           float(beta), _ptr(y), rows, _stream())
    nat.check(rc, "mpcqp_gemv")
    return y


# ------------------------------------------------- bicycle re-linearisation
def bicycle_rti(x0, U, params, ts: float, *, states: bool = False):
    """Batched FE rollout + per-stage linearisation of the kinematic bicycle
    (include/mpcqp.h ``mpcqp_bicycle_rti``).  x0 (b, 4), U (b, N, 2) device
    tensors; params a VehicleParameters.  Returns A (b,N,4,4), B (b,N,4,2),
    c (b,N,4) [, X (b,N+1,4) when states]."""
    dt, dev = x0.dtype, x0.device
    x0 = x0.contiguous()
    U = U.contiguous()
    b, N = int(U.shape[0]), int(U.shape[1])
    A, B, c, X = _alloc({"A": ((b, N, 4, 4), dt), "B": ((b, N, 4, 2), dt), "c": ((b, N, 4), dt),
                         "X": ((b, N + 1, 4), dt) if states else None}, dev)
    prm = _bike_params(params)
    rc = _lib().mpcqp_bicycle_rti(_code(dt), b, N, float(ts), prm, _ptr(x0), 4, _ptr(U), 2 * N,
                                  _ptr(X), _ptr(A), _ptr(B), _ptr(c), _stream())
    nat.check(rc, "mpcqp_bicycle_rti")
    return (A, B, c, X) if states else (A, B, c)


def bicycle_hessian(X, U, pi, params, ts: float, flags=None, mu=None,
                    out: tuple | None = None, Q=None, R=None, eps: float = 1e-6, fix=None,
                    integrator: int = 0):
    """Per stage, the curvature of the dynamics weighted by the costates plus
    a proximal mu I (include/mpcqp.h ``mpcqp_bicycle_hessian``): X (b, N+1,
    4), U (b, N, 2), pi (b, N, 4) fp64, mu (b,) or None -> H2 (b, N, 6, 6),
    q2 (b, N, 6); zeros where flags (b,) lacks SQP_EXACT.  With the stage
    weights Q (4, 4) and R (2, 2): ``mpcqp_bicycle_hessian_convex``, the
    curvature projected so that blkdiag(Q, R) + H2 >= eps I per stage.
    fix (b, N) int32 or None: inputs held at their bound (bits written by
    bicycle_sqp_step) get a proximal term on their diagonal.  integrator:
    the prediction model (0 forward Euler, 1 RK4)."""
    b, N = int(U.shape[0]), int(U.shape[1])
    H2, q2 = _alloc({"H2": ((b, N, 6, 6), torch.float64), "q2": ((b, N, 6), torch.float64)},
                    U.device, out)
    head = (nat.F64, b, N, float(ts), _bike_params(params), int(integrator), _ptr(X), _ptr(U),
            _ptr(pi), _ptr(flags), _ptr(mu), _ptr(fix))
    tail = (_ptr(H2), _ptr(q2), _stream())
    if Q is not None:
        Qc = Q.to(torch.float64).contiguous()
        Rc = R.to(torch.float64).contiguous()
        rc = _lib().mpcqp_bicycle_hessian_convex(*head, _ptr(Qc), _ptr(Rc), float(eps), *tail)
        nat.check(rc, "mpcqp_bicycle_hessian_convex")
        return H2, q2
    rc = _lib().mpcqp_bicycle_hessian(*head, *tail)
    nat.check(rc, "mpcqp_bicycle_hessian")
    return H2, q2


def bicycle_sqp_step(x0, U, Z, yq, piq, y, pi, X, state: dict, params, ts: float, Q, R, Qf,
                     xlo=None, xhi=None, lb=None, ub=None, tol: float = 1e-9, qp_status=None,
                     integrator: int = 0):
    """Line search + update + NLP optimality residual (include/mpcqp.h
    ``mpcqp_bicycle_sqp_step``), in place on U, y, pi, X and ``state``
    (rho, kkt, mu float64 (b,), flags int32 (b,), optional fix int32 (b, N):
    the inputs to hold at their bound in the next exact-Hessian QP).  Bounds: xlo/xhi (N*4,)
    shared or (b, N*4); lb/ub (N*2,) shared or (b, N*2)."""
    b, N = int(U.shape[0]), int(U.shape[1])
    xlo, xhi, sxb = _bound_pair(xlo, xhi, b, 4 * N, "xlo/xhi")
    lb, ub, slb = _bound_pair(lb, ub, b, 2 * N, "lb/ub")
    rc = _lib().mpcqp_bicycle_sqp_step(
        nat.F64, b, N, float(ts), _bike_params(params), int(integrator), _ptr(x0), 4, _ptr(Q),
        _ptr(R), _ptr(Qf),
        _ptr(xlo), _ptr(xhi), sxb, _ptr(lb), _ptr(ub), slb, _ptr(U), _ptr(Z), _ptr(yq), _ptr(piq),
        _ptr(qp_status), _ptr(y), _ptr(pi), _ptr(X), *_sqp_state(state), float(tol), _stream())
    nat.check(rc, "mpcqp_bicycle_sqp_step")


def bicycle_sqp_solve(x0, U, y, pi, X, state: dict, params, ts: float, Q, R, Qf, *,
                      hessian: str = "exact", xlo=None, xhi=None, lb=None, ub=None,
                      tol: float = 1e-9, max_iter: int = 60, qp_max_iter: int = 25,
                      integrator: int = 0, lam_u=None, qp_status=None,
                      ws: torch.Tensor | None = None) -> torch.Tensor:
    """The whole device SQP, up to max_iter iterations per instance, in one
    launch (include/mpcqp.h ``mpcqp_bicycle_sqp_solve``), in place on the SQP
    state U (b, N, 2), y (b, N*4), pi (b, N, 4), X (b, N+1, 4) and ``state``
    (rho, kkt, mu float64 (b,), flags int32 (b,), fix int32 (b, N)) -- the
    state of ``bicycle_sqp_step``, so a solve continues from it.  hessian:
    "exact", "exact-raw" or "gauss-newton".  lam_u (b, N*2) and qp_status
    (b,): optional outputs of the last QP.  Returns the workspace (pass it
    back as ``ws`` to reuse it)."""
    b, N = int(U.shape[0]), int(U.shape[1])
    xlo, xhi, sxb = _bound_pair(xlo, xhi, b, 4 * N, "xlo/xhi")
    lb, ub, slb = _bound_pair(lb, ub, b, 2 * N, "lb/ub")
    f64 = torch.float64
    _check_tensors("bicycle_sqp_solve", U.device,
                   (("U", U, (b, N, 2), f64), ("y", y, (b, N * 4), f64), ("pi", pi, (b, N, 4), f64),
                    ("X", X, (b, N + 1, 4), f64), ("x0", x0, (b, 4), f64)))
    lib = _lib()
    wsb = int(lib.mpcqp_bicycle_sqp_solve_workspace(b, N))
    ws = _workspace(wsb, U.device, ws)
    rc = lib.mpcqp_bicycle_sqp_solve(
        nat.F64, b, N, float(ts), _bike_params(params), int(integrator), nat.SQP_HESS[hessian],
        _ptr(x0), 4, _ptr(Q), _ptr(R), _ptr(Qf), _ptr(xlo), _ptr(xhi), sxb, _ptr(lb), _ptr(ub), slb,
        _ptr(U), _ptr(y), _ptr(pi), _ptr(X), *_sqp_state(state), _ptr(lam_u), _ptr(qp_status),
        int(max_iter), int(qp_max_iter), float(tol), _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_bicycle_sqp_solve")
    return ws


def bicycle_mpc_loop(xs, us, success, iters, state_prediction, input_prediction, U, y, pi, X,
                     state: dict, params, ts: float, Q, R, Qf, *, plant_params, plant: int = 0,
                     substeps: int = 20, hessian: str = "exact", xlo=None, xhi=None, lb=None,
                     ub=None, tol: float = 1e-9, iters_first: int = 60, iters_per_step: int = 10,
                     qp_max_iter: int = 25, integrator: int = 0, mu0: float = 1e-3,
                     ws: torch.Tensor | None = None) -> torch.Tensor:
    """The receding-horizon loop, every sample in one launch (include/mpcqp.h
    ``mpcqp_bicycle_mpc_loop``): xs (T+1, b, 4) with xs[0] given, us (T, b, 2),
    success (T, b) bool, iters (T, b) int32, state_prediction (T, b, N+1, 4),
    input_prediction (T, b, N, 2); the SQP state as ``bicycle_sqp_solve``'s
    (reset before).  Returns the workspace."""
    T, b = int(us.shape[0]), int(U.shape[0])
    N = int(U.shape[1])
    xlo, xhi, sxb = _bound_pair(xlo, xhi, b, 4 * N, "xlo/xhi")
    lb, ub, slb = _bound_pair(lb, ub, b, 2 * N, "lb/ub")
    f64 = torch.float64
    _check_tensors("bicycle_mpc_loop", U.device,
                   (("xs", xs, (T + 1, b, 4), f64), ("us", us, (T, b, 2), f64),
                    ("success", success, (T, b), torch.bool), ("iters", iters, (T, b), torch.int32),
                    ("state_prediction", state_prediction, (T, b, N + 1, 4), f64),
                    ("input_prediction", input_prediction, (T, b, N, 2), f64)))
    lib = _lib()
    wsb = int(lib.mpcqp_bicycle_sqp_solve_workspace(b, N))
    ws = _workspace(wsb, U.device, ws)
    rc = lib.mpcqp_bicycle_mpc_loop(
        nat.F64, b, N, T, float(ts), _bike_params(params), int(integrator), nat.SQP_HESS[hessian],
        _bike_params(plant_params), int(plant), int(substeps), _ptr(Q), _ptr(R), _ptr(Qf),
        _ptr(xlo), _ptr(xhi), sxb, _ptr(lb), _ptr(ub), slb, _ptr(U), _ptr(y), _ptr(pi), _ptr(X),
        *_sqp_state(state), int(iters_first), int(iters_per_step), int(qp_max_iter), float(tol),
        float(mu0), _ptr(xs), _ptr(us), _ptr(success), _ptr(iters), _ptr(state_prediction),
        _ptr(input_prediction), _ptr(ws), wsb, _stream())
    nat.check(rc, "mpcqp_bicycle_mpc_loop")
    return ws


def bicycle_linearise(x0, U, params, ts: float, integrator: int = 0, out: tuple | None = None):
    """Rollout + linearisation of the prediction model (include/mpcqp.h
    ``mpcqp_bicycle_linearise``; integrator 0 = forward Euler, 1 = RK4):
    x0 (b, 4), U (b, N, 2) fp64 -> A (b,N,4,4), B (b,N,4,2), c (b,N,4),
    X (b,N+1,4)."""
    b, N = int(U.shape[0]), int(U.shape[1])
    dev = U.device
    x0, U = x0.contiguous(), U.contiguous()
    f64 = torch.float64
    A, B, c, X = _alloc({"A": ((b, N, 4, 4), f64), "B": ((b, N, 4, 2), f64), "c": ((b, N, 4), f64),
                         "X": ((b, N + 1, 4), f64)}, dev, out)
    rc = _lib().mpcqp_bicycle_linearise(nat.F64, b, N, float(ts), _bike_params(params),
                                        int(integrator), _ptr(x0), 4, _ptr(U), 2 * N, _ptr(X),
                                        _ptr(A), _ptr(B), _ptr(c), _stream())
    nat.check(rc, "mpcqp_bicycle_linearise")
    return A, B, c, X


# --------------------------------------------------------------- rollout
def rollout(A, B, K, x0, steps: int):
    """Closed loop x_{t+1} = (A + B K) x_t for a batch of x0 (b,nx).

    Returns xs (steps, b, nx) time-major; ``xs.permute(2, 1, 0)`` is the
    reference's (nx, batch, steps) state tensor (LinearSystem.py:21,26).
    """
    dt, dev = x0.dtype, x0.device
    A, B, K, x0 = (_dev(v, dt, dev) for v in (A, B, K, x0))
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    batch = int(x0.shape[0])
    xs = torch.empty((steps, batch, nx), dtype=dt, device=dev)
    rc = _lib().mpcqp_rollout(_code(dt), batch, nx, nu, steps, _ptr(A), _ptr(B), _ptr(K), _ptr(x0),
                              _ptr(xs), _stream())
    nat.check(rc, "mpcqp_rollout")
    return xs


def max_qp_size(dtype=torch.float64) -> int:
    """Largest n + m accepted by solve_qp (and n by solve_box) for dtype."""
    return int(_lib().mpcqp_max_qp_size(_code(dtype)))


def n_packed(n: int) -> int:
    return n * (n + 1) // 2


def isqrt_packed(p: int) -> int:
    n = int((math.isqrt(8 * p + 1) - 1) // 2)
    assert n * (n + 1) // 2 == p
    return n
