"""The adjoint of the stand-alone polytope QP on the device
(include/mpcqp_poly_diff.h ``mpcqp_poly_solve_vjp``), on torch tensors with the
conventions of ``batched``.

``poly_solve_vjp`` maps the gradients of a loss with respect to the outputs of
``PolyQP.solve`` -- gz = dL/dz and gy = dL/dy -- to those of its per-instance
operands: gf (the extra gradient f), gx0, and ghl / ghu over all m_total rows of
[G; I], whose rows m.. are the instance's share of dL/dlbz and dL/dubz.
``shared_grads`` forms the gradients of the operands the batch shares (H, F, G,
lbz, ubz) from those, with torch products.

``poly_loop_vjp`` is the same for a whole episode of ``PolyQP.loop``
(include/mpcqp_poly_loop_diff.h ``mpcqp_mpc_poly_loop_vjp``): the reverse-time
recursion over the steps in one launch, from the gradients with respect to xs,
us, zs and ys to gx0, ghl / ghu summed over the episode and the per-step rows
geps, gf = dL/dg_t and gw = dL/dw_t; ``loop_shared_grads`` forms the gradients
of H, F, G, E, the plant A, B and lbz, ubz from those.
"""
from __future__ import annotations

import torch

from . import _native as nat
from . import batched
from .batched import _alloc, _ptr, _stream

__all__ = ["poly_solve_vjp", "scratch_bytes", "shared_grads", "VJP_OUTPUTS",
           "poly_loop_vjp", "loop_scratch_bytes", "loop_shared_grads", "LOOP_VJP_OUTPUTS"]

VJP_OUTPUTS = ("gf", "gx0", "ghl", "ghu")
LOOP_VJP_OUTPUTS = ("gx0", "ghl", "ghu", "geps", "gf", "gw")  # the order of the C prototype
LOOP_SHARED = ("gH", "gF", "gG", "gE", "gA", "gB", "glbz", "gubz")


def _scratch_arg(scratch, nbytes: int, dev):
    """The ``scratch=`` buffer to pass on: a fresh one of ``nbytes`` bytes when
    none was given and some are needed, else the caller's, checked."""
    if scratch is None and nbytes:
        return torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if scratch is not None and (scratch.device.type != "cuda"
                                or scratch.numel() * scratch.element_size() < nbytes):
        raise ValueError(f"scratch must be a device buffer of >= {nbytes} bytes")
    return scratch


def _pack_fold(S):
    """dL/dH on the packed entries from the full, unsymmetrised S = sum gf z':
    (i, j<i) = S_ij + S_ji, (i, i) = S_ii."""
    St = S + S.transpose(0, 1)
    St = St - torch.diag(torch.diagonal(S))
    return batched.pack_lower(St)


def _row_grads(qp, need, z, y, gf, e, x=None, u=None, gw=None) -> dict:
    """The shared operands' gradients as sums over flattened rows (one per
    instance, or per step and instance; failed ones already zeroed): gH, gG,
    glbz, gubz, with ``x`` gF and gE, with ``gw`` gA and gB.  An entry not in
    ``need``, or whose operand ``qp`` does not have, is None."""
    m, o = qp.m, dict.fromkeys(LOOP_SHARED)
    if "gH" in need:
        o["gH"] = _pack_fold(gf.transpose(0, 1) @ z)
    if "gF" in need and x is not None:
        o["gF"] = gf.transpose(0, 1) @ x
    if "gG" in need and m > 0:
        o["gG"] = y[:, :m].transpose(0, 1) @ gf - e[:, :m].transpose(0, 1) @ z
    if "gE" in need and m > 0:
        o["gE"] = -(e[:, :m].transpose(0, 1) @ x)
    if "gA" in need:
        o["gA"] = gw.transpose(0, 1) @ x
    if "gB" in need:
        o["gB"] = gw.transpose(0, 1) @ u
    if qp.nbox and "glbz" in need:
        o["glbz"] = torch.where(y[:, m:] < 0, e[:, m:], torch.zeros_like(e[:, m:])).sum(0)
    if qp.nbox and "gubz" in need:
        o["gubz"] = torch.where(y[:, m:] > 0, e[:, m:], torch.zeros_like(e[:, m:])).sum(0)
    return o


def scratch_bytes(qp, batch: int) -> int:
    """Bytes of the ``scratch=`` buffer of ``poly_solve_vjp`` for ``batch``
    instances of ``qp`` (``mpcqp_poly_solve_vjp_workspace``)."""
    return int(batched._lib().mpcqp_poly_solve_vjp_workspace(
        batched._code(qp.dtype), int(batch), qp.n, qp.m, qp.nbox))


def poly_solve_vjp(qp, y, gz=None, gy=None, *, status=None, need=VJP_OUTPUTS, scratch=None) -> dict:
    """Adjoint of ``qp.solve`` (a ``batched.PolyQP``) at its optimum, two
    launches.  ``y`` (b, m_total) and ``status`` (b,) are what ``solve``
    returned (status None: every instance counts as OPTIMAL); ``gz`` (b, n) and
    ``gy`` (b, m_total) are dL/dz and dL/dy, None meaning zero.  Returns a dict
    with the entries of ``need`` (the others None) out of

    * ``gf`` (b, n) = dL/df, ``gx0`` (b, nx) = dL/dx0 (only for a ``qp`` with F),
      ``ghl``, ``ghu`` (b, m_total) = dL/dhl, dL/dhu on the rows below m and the
      instance's dL/dlbz, dL/dubz on the rows from m on,

    ``e`` = ghl + ghu when both were asked for (the adjoint's row variable, what
    ``shared_grads`` takes) and ``vstatus`` (b,) int32: a bare STATUS_* code,
    the forward's if that is not OPTIMAL, else NOT_CONVEX (H not positive
    definite, or the rows marked active are dependent), NONFINITE, or OPTIMAL.
    Every gradient of an instance whose vstatus is not OPTIMAL is exactly zero.
    ``scratch``: a preallocated uint8 device buffer of ``scratch_bytes(qp, b)``
    bytes (for graph capture); None allocates one when gz is given."""
    dt, dev = qp.dtype, qp.ws.device
    unknown = set(need) - set(VJP_OUTPUTS)
    if unknown:
        raise ValueError(f"need: unknown outputs {sorted(unknown)}")
    if "gx0" in need and qp.nx == 0:
        raise ValueError("gx0 asked for, but this PolyQP has no x0 -> gradient map F")
    y = batched._dev(y, dt, dev)
    if y.ndim != 2 or y.shape[1] != qp.mt:
        raise ValueError(f"y must be (batch, {qp.mt}), got {tuple(y.shape)}")
    batch = int(y.shape[0])
    gz, gy = batched._dev(gz, dt, dev), batched._dev(gy, dt, dev)
    for name, t, w in (("gz", gz, qp.n), ("gy", gy, qp.mt)):
        if t is not None and tuple(t.shape) != (batch, w):
            raise ValueError(f"{name} must be ({batch}, {w}), got {tuple(t.shape)}")
    if status is not None and (status.dtype != torch.int32 or tuple(status.shape) != (batch,)
                               or not status.is_contiguous()):
        raise ValueError(f"status must be a contiguous int32 tensor of shape ({batch},)")
    shapes = dict(gf=(batch, qp.n), gx0=(batch, qp.nx), ghl=(batch, qp.mt), ghu=(batch, qp.mt))
    o = _alloc({**{k: (shapes[k], dt) if k in need else None for k in VJP_OUTPUTS},
                "vstatus": ((batch,), torch.int32)}, dev, keyed=True)
    scratch = _scratch_arg(scratch, scratch_bytes(qp, batch) if gz is not None else 0, dev)
    rc = batched._lib().mpcqp_poly_solve_vjp(
        batched._code(dt), batch, qp.n, qp.m, qp.nbox, qp.nx, _ptr(qp.ws), _ptr(y), _ptr(status),
        _ptr(gz), _ptr(gy), *(_ptr(o[k]) for k in VJP_OUTPUTS), _ptr(o["vstatus"]),
        _ptr(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size(),
        _stream())
    nat.check(rc, "mpcqp_poly_solve_vjp")
    o["e"] = o["ghl"] + o["ghu"] if o["ghl"] is not None and o["ghu"] is not None else None
    return o


def shared_grads(qp, x0, z, y, gf, e, vstatus, need=("gH", "gF", "gG", "glbz", "gubz")) -> dict:
    """The gradients of the operands of ``qp`` that the batch shares, from the
    per-instance results of ``poly_solve_vjp`` (``gf``, ``e`` = ghl + ghu,
    ``vstatus``) and the forward's ``x0`` (b, nx) or (nx,) or None, ``z`` and
    ``y``.  With S = sum_b gf_b z_b':

    * ``gH`` on the packed entries, folded as ``batched.solve_box_vjp`` does:
      (i, j<i) = S_ij + S_ji, (i, i) = S_ii;
    * ``gF`` (n, nx) = sum_b gf_b x0_b' (zeros without x0; None without F);
    * ``gG`` (m, n) = the rows below m of sum_b (y_b gf_b' - e_b z_b') (None for m = 0);
    * ``glbz``, ``gubz`` (n,) = the sums of e over the box rows held at their
      lower / upper side (None without a box).

    The rows of z, y (and x0) of every instance whose vstatus is not OPTIMAL are
    zeroed first: the forward wrote NaN there, and 0 * NaN would poison the sums."""
    ok = (vstatus == nat.STATUS_OPTIMAL)[:, None]
    batch = int(z.shape[0])

    def keep(t):
        return torch.where(ok, t, torch.zeros_like(t))

    names = ("gH", "gF", "gG", "glbz", "gubz")
    gF = "gF" in need and qp.nx > 0
    x = keep(x0.expand(batch, qp.nx)) if gF and x0 is not None else None
    o = _row_grads(qp, set(need) & set(names), keep(z), keep(y), keep(gf), keep(e), x)
    o = {k: o[k] for k in names}
    if gF and x0 is None:
        o["gF"] = torch.zeros((qp.n, qp.nx), dtype=z.dtype, device=z.device)
    return o


# ------------------------------------------------ the one-launch loop
def loop_scratch_bytes(qp, batch: int, steps: int) -> int:
    """Bytes of the ``scratch=`` buffer of ``poly_loop_vjp`` with gzs, for an
    episode of ``steps`` steps of ``batch`` instances of ``qp``
    (``mpcqp_mpc_poly_loop_vjp_workspace``)."""
    return int(batched._lib().mpcqp_mpc_poly_loop_vjp_workspace(
        batched._code(qp.dtype), int(batch), qp.n, qp.m, qp.nbox, int(steps)))


def poly_loop_vjp(qp, A, B, ys, gxs=None, gus=None, gzs=None, gys=None, *, E=None, status=None,
                  need=LOOP_VJP_OUTPUTS, scratch=None) -> dict:
    """Adjoint of a whole episode of ``qp.loop`` (a ``batched.PolyQP``; hard,
    with or without g / e), the reverse-time recursion in one launch (two with
    gzs): include/mpcqp_poly_loop_diff.h ``mpcqp_mpc_poly_loop_vjp``.  ``A``
    (nx, nx), ``B`` (nx, nu) and ``E`` (m, nx) or None are the plant and the row
    shift the forward ran with; ``ys`` (T, b, m_total) and ``status`` (T, b)
    what it returned (status None: every step counts as OPTIMAL); ``gxs``
    (T+1, b, nx), ``gus`` (T, b, nu), ``gzs`` (T, b, n), ``gys`` (T, b, m_total)
    the gradients of the loss with respect to xs, us, zs, ys, None meaning
    zero.  Returns a dict with the entries of ``need`` (the others None) out of

    * ``gx0`` (b, nx) = dL/dx0; ``ghl``, ``ghu`` (b, m_total), summed over the
      episode: dL/dhl, dL/dhu on the rows below m and the instance's dL/dlbz,
      dL/dubz on the rows from m on;
    * ``geps`` (T, b, m_total), the row variable eps_t of every step (dL/de_t
      = -geps[t][:, :m]); ``gf`` (T, b, n) = dL/dg_t; ``gw`` (T, b, nx) = dL/dw_t,

    and ``vstatus`` (b,) int32: a bare STATUS_* code, the forward's at the first
    step that did not end OPTIMAL (INFEASIBLE for a softened step), else
    NOT_CONVEX (H not positive definite, or dependent active rows at some
    step), NONFINITE, or OPTIMAL.  Every gradient of an instance whose vstatus
    is not OPTIMAL is exactly zero, its per-step rows included.  ``scratch``: a
    preallocated uint8 device buffer of ``loop_scratch_bytes(qp, b, T)`` bytes
    (for graph capture); None allocates one when gzs is given."""
    dt, dev = qp.dtype, qp.ws.device
    unknown = set(need) - set(LOOP_VJP_OUTPUTS)
    if unknown:
        raise ValueError(f"need: unknown outputs {sorted(unknown)}")
    n, m, mt, nx = qp.n, qp.m, qp.mt, qp.nx
    if nx == 0:
        raise ValueError("poly_loop_vjp needs a PolyQP with the x0 -> gradient map F")
    A, B, E = batched._dev(A, dt, dev), batched._dev(B, dt, dev), batched._dev(E, dt, dev)
    if tuple(A.shape) != (nx, nx):
        raise ValueError(f"A must be ({nx}, {nx}), got {tuple(A.shape)}")
    if B.ndim != 2 or B.shape[0] != nx:
        raise ValueError(f"B must be ({nx}, nu), got {tuple(B.shape)}")
    nu = int(B.shape[1])
    if E is not None and tuple(E.shape) != (m, nx):
        raise ValueError(f"E must be ({m}, {nx}), got {tuple(E.shape)}")
    ys = batched._dev(ys, dt, dev)
    if ys.ndim != 3 or ys.shape[2] != mt:
        raise ValueError(f"ys must be (steps, batch, {mt}), got {tuple(ys.shape)}")
    T, batch = int(ys.shape[0]), int(ys.shape[1])
    gxs, gus, gzs, gys = (batched._dev(g, dt, dev) for g in (gxs, gus, gzs, gys))
    for name, t, shape in (("gxs", gxs, (T + 1, batch, nx)), ("gus", gus, (T, batch, nu)),
                           ("gzs", gzs, (T, batch, n)), ("gys", gys, (T, batch, mt))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if status is not None and (status.dtype != torch.int32 or tuple(status.shape) != (T, batch)
                               or not status.is_contiguous()):
        raise ValueError(f"status must be a contiguous int32 tensor of shape ({T}, {batch})")
    shapes = dict(gx0=(batch, nx), ghl=(batch, mt), ghu=(batch, mt), geps=(T, batch, mt),
                  gf=(T, batch, n), gw=(T, batch, nx))
    o = _alloc({**{k: (shapes[k], dt) if k in need else None for k in LOOP_VJP_OUTPUTS},
                "vstatus": ((batch,), torch.int32)}, dev, keyed=True)
    scratch = _scratch_arg(scratch, loop_scratch_bytes(qp, batch, T) if gzs is not None else 0, dev)
    rc = batched._lib().mpcqp_mpc_poly_loop_vjp(
        batched._code(dt), batch, n, m, qp.nbox, nx, nu, T, _ptr(qp.ws), _ptr(E), _ptr(A), _ptr(B),
        _ptr(ys), _ptr(status), _ptr(gxs), _ptr(gus), _ptr(gzs), _ptr(gys),
        *(_ptr(o[k]) for k in LOOP_VJP_OUTPUTS), _ptr(o["vstatus"]), _ptr(scratch),
        0 if scratch is None else scratch.numel() * scratch.element_size(), _stream())
    nat.check(rc, "mpcqp_mpc_poly_loop_vjp")
    return o


def loop_shared_grads(qp, xs, us, zs, ys, gf, geps, gw, vstatus, need=LOOP_SHARED) -> dict:
    """The gradients of the operands an episode shares over its steps and
    instances, from the per-step results of ``poly_loop_vjp`` (``gf``, ``geps``,
    ``gw``, ``vstatus``) and the forward's ``xs`` (T+1, b, nx), ``us``, ``zs``,
    ``ys``: sums over all (t, b) rows.  With S = sum gf_t z_t':

    * ``gH`` on the packed entries, folded: (i, j<i) = S_ij + S_ji, (i, i) = S_ii;
    * ``gF`` (n, nx) = sum gf_t x_t';
    * ``gG`` (m, n) = the rows below m of sum (y_t gf_t' - eps_t z_t'), ``gE`` (m,
      nx) = -sum eps_t[:m] x_t' (both None for m = 0);
    * ``gA`` (nx, nx) = sum gw_t x_t', ``gB`` (nx, nu) = sum gw_t u_t';
    * ``glbz``, ``gubz`` (n,) = the sums of eps over the box rows held at their
      lower / upper side (None without a box).

    An entry of ``need`` whose per-step input (gf, geps or gw) is None raises.
    The rows of every instance whose vstatus is not OPTIMAL are zeroed first:
    the forward wrote NaN there, and 0 * NaN would poison the sums."""
    unknown = set(need) - set(LOOP_SHARED)
    if unknown:
        raise ValueError(f"need: unknown gradients {sorted(unknown)}")
    uses = dict(gH=("gf",), gF=("gf",), gG=("gf", "geps"), gE=("geps",), gA=("gw",), gB=("gw",),
                glbz=("geps",), gubz=("geps",))
    given = dict(gf=gf, geps=geps, gw=gw)
    for k in need:
        for u in uses[k]:
            if given[u] is None:
                raise ValueError(f"{k} needs {u}")
    ok = (vstatus == nat.STATUS_OPTIMAL)[None, :, None]
    T, n, nx = int(ys.shape[0]), qp.n, qp.nx

    def rows(t, width):
        """(T * b, width) with the rows of failed instances zeroed"""
        return None if t is None else torch.where(ok, t, torch.zeros_like(t)).reshape(-1, width)

    x, u = rows(xs[:T], nx), rows(us, int(us.shape[-1]))
    z, y = rows(zs, n), rows(ys, qp.mt)
    return _row_grads(qp, need, z, y, rows(gf, n), rows(geps, qp.mt), x, u, rows(gw, nx))
