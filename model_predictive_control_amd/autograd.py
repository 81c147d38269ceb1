"""Differentiable box QP and box-MPC step (torch.autograd).

The forward passes are ``batched.solve_box`` and ``batched.mpc_box``
unchanged; the backward passes run the adjoint kernel of
``batched.solve_box_vjp`` (include/mpcqp.h ``mpcqp_solve_box_vjp``).  With
g = dL/dz, F the free rows of the optimum z and A the rows at a bound
(compared exactly):

    d_F  = -H_FF^-1 g_F,  d_A = 0            dL/df = d
    nu_A = g_A + H_AF d_F                    dL/dlb, dL/dub on the side held
    dL/dH = d z'                             folded onto the packed entries

A row at a bound with a zero multiplier counts as active, so there the result
is the one-sided derivative that keeps the row at its bound.  An instance whose
forward solve did not end OPTIMAL (or whose adjoint meets a NaN or a
non-positive pivot) contributes exact zeros to every gradient.  n <= 32.

``box_loop_diff`` and ``mpc_box_loop_diff`` are the same for a whole
closed-loop episode: the forward is ``batched.mpc_box_loop`` (one launch), the
backward one launch of ``batched.mpc_box_loop_vjp`` (include/mpcqp.h
``mpcqp_mpc_box_loop_vjp``), the reverse-time recursion

    lam <- gxs[T];  for t = T-1 .. 0:  gz = gzs[t] (+ gus[t] + B'lam on u_t),
    d, nu as above at z_t,  dL/dg_t = d,  dL/dw_t = lam,  dL/dH += d z_t',
    dL/dF += d x_t',  dL/dA += lam x_t',  dL/dB += lam u_t',
    lam <- gxs[t] + A'lam + F'd;   dL/dx0 = lam

with the same conventions; an instance with a step that did not end OPTIMAL
contributes exact zeros.  nx <= 4, nu <= 2, n <= 32.

``condense_diff``, ``mpc_box_model_diff`` and ``mpc_box_loop_model_diff`` carry
the graph on to the prediction model: their backward passes end in one launch
of ``condense_diff.condense_vjp`` (include/mpcqp_diff.h ``mpcqp_condense_vjp``),
the adjoint of the condensing recursion, which maps dL/dH, dL/dF and dL/df to
A, B, c, Q, R, Qf and x0.  Same limits.

``poly_solve_diff`` and ``mpc_poly_diff`` are the state-constrained half: the
forward is ``batched.PolyQP.solve`` unchanged, the backward the adjoint of
``poly_diff.poly_solve_vjp`` (include/mpcqp_poly_diff.h ``mpcqp_poly_solve_vjp``).
With the active rows A = {i : y_i != 0} of C = [G; I], gz = dL/dz and gy = dL/dy:

    e_A = M_AA^-1 (C Hinv gz - gy)_A,  dL/df = -Hinv (gz - C_A' e_A),
    dL/dx0 = F' dL/df,  dL/dhl, dL/dhu = e on the side held,
    dL/dH = dL/df z',  dL/dF = dL/df x0',  dL/dG = y dL/df' - e z'

A row at its bound with a zero multiplier counts as inactive (the one-sided
derivative on the side that lets it leave).  m_total <= 64, nx <= 16.

``poly_loop_diff`` and ``mpc_poly_loop_diff`` are the same for a whole
state-constrained episode: the forward is ``batched.PolyQP.loop`` (one launch),
the backward one launch of ``poly_diff.poly_loop_vjp``
(include/mpcqp_poly_loop_diff.h ``mpcqp_mpc_poly_loop_vjp``; a second launch
before it when the loss reads zs), the reverse-time recursion

    lam <- gxs[T];  for t = T-1 .. 0:  gz = gzs[t] (+ gus[t] + B'lam on u_t),
    eps_t, dL/dg_t as e, dL/df above at (z_t, y_t),  dL/de_t = -eps_t,
    dL/dw_t = lam,  lam <- gxs[t] + A'lam + F' dL/dg_t - E' eps_t;  dL/dx0 = lam

with the shared operands' gradients summed over the steps and the batch.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import batched
from . import condense_diff as _cdiff
from . import poly_diff as _pdiff

__all__ = ["solve_box_diff", "mpc_box_diff", "box_loop_diff", "mpc_box_loop_diff",
           "condense_diff", "mpc_box_model_diff", "mpc_box_loop_model_diff",
           "poly_solve_diff", "mpc_poly_diff", "poly_loop_diff", "mpc_poly_loop_diff"]

MAX_N = batched.BOX_VJP_MAX_N


def _needs(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _like_input(g, ref):
    """The gradient ``g`` (shared: (n,), batched: (b, n)) in the shape of the
    bound tensor ``ref`` it belongs to (a 0-dim bound is spread over the rows)."""
    if ref.ndim == 0:
        return g.sum()
    return g.reshape(ref.shape)


def _stash(ctx, tensors, optional):
    """Save for backward: ``tensors``, and of the optional inputs those that
    are tensors; anything else among them (None, a Python scalar) stays on
    ``ctx``."""
    ctx.opt_plain = [None if isinstance(t, torch.Tensor) else t for t in optional]
    ctx.opt_tensor = [isinstance(t, torch.Tensor) for t in optional]
    ctx.save_for_backward(*tensors, *(t for t in optional if isinstance(t, torch.Tensor)))


def _recover(ctx, k):
    """The ``k`` tensors and the optional inputs of ``_stash``, in its order."""
    saved = list(ctx.saved_tensors)
    rest = saved[k:]
    return saved[:k] + [rest.pop(0) if fl else pl for fl, pl in zip(ctx.opt_tensor, ctx.opt_plain)]


def _bound_grad(g, bound, needed):
    """The gradient of a bound given as a tensor, in its shape; None otherwise."""
    return _like_input(g, bound) if isinstance(bound, torch.Tensor) and needed else None


class _SolveBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, f, lb, ub, kw):
        z, status = batched.solve_box(H, f, lb, ub, **kw)
        ctx.mark_non_differentiable(status)
        _stash(ctx, (H, f, z, status), (lb, ub))
        return z, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _gstatus):
        H, f, z, status, lb, ub = _recover(ctx, 4)
        need = ctx.needs_input_grad
        r = batched.solve_box_vjp(H, z, lb, ub, gz.to(z.dtype), status=status, need_H=need[0])
        gH = r["gH"] if need[0] else None
        gf = None
        if need[1]:
            gf = r["gf"] if f.ndim == 2 else r["gf"].sum(0)
        return gH, gf, _bound_grad(r["glb"], lb, need[2]), _bound_grad(r["gub"], ub, need[3]), None


def solve_box_diff(H, f, lb=None, ub=None, **kw):
    """``batched.solve_box`` with gradients: returns ``(z, status)`` where z
    carries the graph to packed H, f and tensor lb / ub (Python-scalar bounds
    get none) and status is non-differentiable.  Keyword arguments go to
    ``solve_box``.  The gradient of a shared input is summed over the batch."""
    n = int(f.shape[-1])
    if n > MAX_N and _needs(H, f, lb, ub):
        raise NotImplementedError(
            f"solve_box_diff: gradients are limited to n <= {MAX_N}, got n = {n}")
    return _SolveBox.apply(H, f, lb, ub, kw)


def _sym(M):
    return 0.5 * (M + M.transpose(-1, -2))


class _MpcBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, Q, R, Qf, x0, lb, ub, c, N, tv, kw):
        z, status = batched.mpc_box(A, B, Q, R, Qf, N, x0, lb, ub, c, tv=tv, **kw)
        ctx.mark_non_differentiable(status)
        _stash(ctx, (A, B, Q, R, Qf, x0, z, status), (lb, ub, c))
        ctx.N, ctx.tv = N, tv
        return z, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _gstatus):
        A, B, Q, R, Qf, x0, z, status, lb, ub, c = _recover(ctx, 8)
        need = ctx.needs_input_grad
        N = ctx.N
        nx, nu = int(B.shape[-2]), int(B.shape[-1])
        batch, n = z.shape
        cd = batched.condense(A, B, Q, R, Qf, N, x0=x0, c=c, tv=ctx.tv,
                              outputs=("H", "F", "Gam", "xbar"))
        H, F, Gam, xbar = cd["H"], cd["F"], cd["Gam"], cd["xbar"]
        # one condensed problem for the whole batch when only the bounds vary
        r = batched.solve_box_vjp(H[0] if H.shape[0] == 1 and batch > 1 else H, z, lb, ub,
                                  gz.to(z.dtype), status=status, need_H=False)
        d = r["gf"]
        ok = (r["vstatus"] == 0)[:, None]
        zc = torch.where(ok, z, torch.zeros_like(z))  # failed instances: z may be NaN, d is 0
        gx0 = gQ = gR = gQf = None

        def keep(g):
            # The zero-gradient rule for the products below: a failed instance
            # has d = 0, but its F, Gam or xbar may hold NaN (a non-finite x0,
            # A or B), and 0 * NaN is NaN: select, per instance, before any
            # sum over the batch.
            return torch.where(ok.reshape((batch,) + (1,) * (g.ndim - 1)), g, torch.zeros_like(g))

        if need[5]:
            gx0 = keep(torch.einsum("bij,bi->bj", F.expand(batch, -1, -1), d))
            if x0.ndim == 1:
                gx0 = gx0.sum(0)
        if need[2] or need[4]:
            Gb = Gam.expand(batch, -1, -1)
            dX = torch.einsum("bij,bj->bi", Gb, d).reshape(batch, N, nx)
            X = (xbar.expand(batch, -1) + torch.einsum("bij,bj->bi", Gb, zc)).reshape(batch, N, nx)
            if need[2]:
                gQ = keep(_sym(torch.einsum("bki,bkj->bij", dX[:, :N - 1], X[:, :N - 1])))
                if Q.ndim == 2:
                    gQ = gQ.sum(0)
            if need[4]:
                gQf = keep(_sym(dX[:, N - 1, :, None] * X[:, N - 1, None, :]))
                if Qf.ndim == 2:
                    gQf = gQf.sum(0)
        if need[3]:
            gR = keep(_sym(torch.einsum("bki,bkj->bij", d.reshape(batch, N, nu),
                                        zc.reshape(batch, N, nu))))
            if R.ndim <= 2:
                gR = gR.sum(0)
            gR = gR.reshape(R.shape)
        glb, gub = _bound_grad(r["glb"], lb, need[6]), _bound_grad(r["gub"], ub, need[7])
        return None, None, gQ, gR, gQf, gx0, glb, gub, None, None, None, None


def mpc_box_diff(A, B, Q, R, Qf, N, x0, lb=None, ub=None, c=None, *, tv=False, **kw):
    """``batched.mpc_box`` (the fused condense + box-QP kernel) with gradients:
    returns ``(z, status)`` where z carries the graph to x0, Q, R, Qf and tensor
    lb / ub.  The backward pass condenses the instances (``batched.condense``),
    runs the adjoint kernel for d = dL/df and nu, and maps them back:
    grad_x0 = F'd, and with dX = Gam d, X = xbar + Gam z over the stages,
    grad_Q = sym(sum_{k<N-1} dX_k X_k'), grad_Qf = sym(dX_{N-1} X_{N-1}'),
    grad_R = sym(sum_k d_k z_k'), summed over the batch for a shared weight.
    Gradients through A, B or c (the condensing recursion) are not provided."""
    if _needs(A, B, c):
        raise NotImplementedError(
            "mpc_box_diff: gradients through A, B and c (the condensing recursion) are not "
            "implemented; detach them")
    n = int(N) * int(B.shape[-1])
    if n > MAX_N and _needs(Q, R, Qf, x0, lb, ub):
        raise NotImplementedError(
            f"mpc_box_diff: gradients are limited to N * nu <= {MAX_N}, got {n}")
    return _MpcBox.apply(A, B, Q, R, Qf, x0, lb, ub, c, int(N), bool(tv), kw)


class _BoxLoop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, F, A, B, x0, lb, ub, g, w, steps, kw):
        nu = int(B.shape[-1])
        N = int(F.shape[-2]) // nu
        o = batched.mpc_box_loop(A, B, None, None, None, N, x0, lb, ub, steps, plans=True,
                                 condensed={"H": H, "F": F}, g=g, w=w, **kw)
        xs, us, zs, status = o["xs"], o["us"], o["zs"], o["status"]
        ctx.mark_non_differentiable(status)
        ctx.set_materialize_grads(False)
        _stash(ctx, (H, F, A, B, xs, zs, status), (lb, ub, g))
        return xs, us, zs, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gxs, gus, gzs, _gstatus):
        H, F, A, B, xs, zs, status, lb, ub, g = _recover(ctx, 7)
        need = ctx.needs_input_grad  # H, F, A, B, x0, lb, ub, g, w
        names = ("gH", "gF", "gA", "gB", "gx0", "glb", "gub", "gg", "gw")
        want = tuple(k for k, nd in zip(names, need) if nd)
        dt = zs.dtype
        r = batched.mpc_box_loop_vjp(H, F, A, B, lb, ub, xs, zs,
                                     *(None if t is None else t.to(dt) for t in (gxs, gus, gzs)),
                                     status=status, need=want)
        glb, gub = _bound_grad(r["glb"], lb, need[5]), _bound_grad(r["gub"], ub, need[6])
        gg = r["gg"]
        if gg is not None and g.ndim == 2:  # shared by the batch
            gg = gg.sum(1)
        return r["gH"], r["gF"], r["gA"], r["gB"], r["gx0"], glb, gub, gg, r["gw"], None, None


def box_loop_diff(H, F, A, B, x0, lb=None, ub=None, *, steps, g=None, w=None, cold=False,
                  max_iter=0, tol=0.0):
    """``batched.mpc_box_loop`` on a condensed problem (packed H, F: f_t = F x_t
    + g_t) with gradients: returns ``(xs, us, zs, status)`` where xs (T+1, b,
    nx), us (T, b, nu) and zs (T, b, n) carry the graph to H, F, the plant A, B
    of the simulation, x0 (b, nx), tensor lb / ub, g ((T, n) shared: summed over
    the batch, or (T, b, n)) and w (T, b, nx); status is non-differentiable.
    The forward is ``mpc_box_loop(..., condensed={"H": H, "F": F}, plans=True)``
    unchanged, the backward one launch of ``batched.mpc_box_loop_vjp``.  H and F
    are independent inputs here: no gradient flows from them to A and B (the
    condensing recursion is not differentiated)."""
    kw = dict(cold=bool(cold), max_iter=int(max_iter), tol=float(tol))
    return _BoxLoop.apply(H, F, A, B, x0, lb, ub, g, w, int(steps), kw)


def mpc_box_loop_diff(A, B, Q, R, Qf, N, x0, lb=None, ub=None, *, steps, x_ref=None, u_ref=None,
                      w=None, cold=False, max_iter=0, tol=0.0):
    """``batched.mpc_box_loop`` (the one-launch input-box MPC episode, with
    reference tracking and disturbances) with gradients: returns ``(xs, us, zs,
    status)``, bit for bit the values of ``mpc_box_loop(..., plans=True)``,
    where xs, us, zs carry the graph to the shared weights Q, R, Qf, to x0, to
    tensor lb / ub, to w and to the references.  The plant is condensed once
    (``batched.condense``); the graph to the weights is carried by torch
    expressions on the detached Gam, Phi of that call,

        H = Gam' Qhat Gam + Rhat,  F = Gam' Qhat Phi,  g = tracking_terms(...)

    attached to the kernel's own H and F as value + (expr - expr.detach()), and
    ``box_loop_diff`` does the rest.  Gradients of the weights are symmetric.
    Gradients through A or B (the condensing recursion) are not provided; those
    of the simulated plant alone are what ``box_loop_diff`` gives."""
    if _needs(A, B):
        raise NotImplementedError(
            "mpc_box_loop_diff: gradients through A and B (the condensing recursion) are not "
            "implemented; detach them, or use box_loop_diff for the simulated plant's")
    N, T = int(N), int(steps)
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    tracking = x_ref is not None or u_ref is not None
    dt, dev = A.dtype, A.device
    wts = [torch.as_tensor(v, dtype=dt, device=dev) for v in (Q, R, Qf)]
    Q, R, Qf = wts[0], batched._weight_r(wts[1], nu), wts[2]
    if Q.ndim != 2 or R.ndim != 2 or Qf.ndim != 2:
        raise NotImplementedError("mpc_box_loop_diff: Q, R, Qf must be shared by the batch")
    det = [v.detach() for v in (Q, R, Qf)]
    if _needs(Q, R, Qf):
        # the value of each weight with the graph of its symmetric part
        Q, R, Qf = (v.detach() + (_sym(v) - _sym(v).detach()) for v in (Q, R, Qf))
    # the condensing call of mpc_box_loop itself (its H and F are the values)
    cd = batched.condense(A, B, *det, N, outputs=("H", "F", "Gam") if tracking else ("H", "F"))
    H, F = cd["H"], cd["F"]
    g = None
    if _needs(Q, R, Qf):
        aux = batched.condense(A, B, *det, N, outputs=("Gam", "Phi"))
        Gam, Phi = aux["Gam"], aux["Phi"]
        Qhat = torch.block_diag(*([Q] * (N - 1) + [Qf]))
        Rhat = torch.block_diag(*([R] * N))
        GQ = Gam.transpose(-1, -2) @ Qhat
        He = batched.pack_lower(GQ @ Gam + Rhat)
        Fe = GQ @ Phi
        H = H + (He - He.detach())
        F = F + (Fe - Fe.detach())
    if tracking:
        Gam = cd["Gam"]
        if Gam.ndim == 3 and Gam.shape[0] == 1:
            Gam = Gam[0]
        g = batched.tracking_terms({"Gam": Gam}, Q, R, Qf, N, T, x_ref, u_ref)
    return box_loop_diff(H, F, A, B, x0, lb, ub, steps=T, g=g, w=w, cold=cold, max_iter=max_iter,
                         tol=tol)


# ------------------------------------------------ gradients of the model
_COND_DIFF = ("H", "F", "f")  # the outputs of condensing that mpcqp_condense_vjp takes back


def _r_matrix(R, nu: int):
    """R as a matrix, by torch operations that carry its graph: a 0-dim R is
    R I (its gradient is the trace of the matrix's), a vector the diagonal."""
    if R.ndim == 0:
        return R * torch.eye(nu, dtype=R.dtype, device=R.device)
    if R.ndim == 1:
        if R.shape[0] != nu:
            raise ValueError(f"R of shape {tuple(R.shape)} with nu={nu}")
        return torch.diag(R)
    return R


def _model_limits(who: str, nx: int, nu: int, n: int):
    if nx > _cdiff.MAX_NX or nu > _cdiff.MAX_NU or n > _cdiff.MAX_N:
        raise NotImplementedError(
            f"{who}: gradients are limited to nx <= {_cdiff.MAX_NX}, nu <= {_cdiff.MAX_NU}, "
            f"N * nu <= {_cdiff.MAX_N}, got nx = {nx}, nu = {nu}, N * nu = {n}")


def _plant_tensors(A, B, Q, R, Qf):
    """A, B, Q, R (a matrix), Qf as tensors of A's dtype on its device."""
    dt, dev = A.dtype, A.device
    A, B, Q, R, Qf = (torch.as_tensor(v, dtype=dt, device=dev) for v in (A, B, Q, R, Qf))
    return A, B, Q, _r_matrix(R, int(B.shape[-1])), Qf


class _Condense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, Q, R, Qf, x0, c, N, tv, outputs):
        cd = batched.condense(A, B, Q, R, Qf, N, x0=x0, c=c, tv=tv, outputs=outputs)
        out = tuple(cd[k] for k in outputs)
        ctx.mark_non_differentiable(*(v for k, v in zip(outputs, out) if k not in _COND_DIFF))
        ctx.set_materialize_grads(False)
        _stash(ctx, (A, B, Q, R, Qf), (x0, c))
        ctx.N, ctx.tv, ctx.outputs = N, tv, outputs
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        A, B, Q, R, Qf, x0, c = _recover(ctx, 5)
        names = ("gA", "gB", "gQ", "gR", "gQf", "gx0", "gc")
        want = tuple(k for k, nd in zip(names, ctx.needs_input_grad) if nd)
        up = {k: None if g is None else g.to(A.dtype) for k, g in zip(ctx.outputs, gs)}
        r = _cdiff.condense_vjp(A, B, Q, R, Qf, ctx.N, x0, c, tv=ctx.tv, gH=up.get("H"),
                                gF=up.get("F"), gf=up.get("f"), need=want)
        return (*(r[k] for k in names), None, None, None)


def condense_diff(A, B, Q, R, Qf, N, x0=None, c=None, *, tv=False, outputs=("H", "F", "f")):
    """``batched.condense`` with gradients: returns the requested ``outputs``
    (among H (packed), F, f), in that order, bit for bit those of
    ``batched.condense``, carrying the graph to A, B, Q, R, Qf, c and x0.  The
    backward pass is one launch of ``condense_diff.condense_vjp``; the gradient
    of a shared input is summed over the batch, those of Q, R, Qf are symmetric.
    R may be a matrix, a 0-dim tensor (R I: its gradient is the trace) or a
    vector (the diagonal).  nx <= 4, nu <= 2, N * nu <= 32."""
    outputs = tuple(outputs)
    if set(outputs) - set(_COND_DIFF):
        raise ValueError(f"condense_diff: outputs are among {_COND_DIFF}, got {outputs}")
    A, B, Q, R, Qf = _plant_tensors(A, B, Q, R, Qf)
    if _needs(A, B, Q, R, Qf, x0, c):
        _model_limits("condense_diff", int(B.shape[-2]), int(B.shape[-1]), int(N) * int(B.shape[-1]))
    return _Condense.apply(A, B, Q, R, Qf, x0, c, int(N), bool(tv), outputs)


class _MpcBoxModel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, Q, R, Qf, x0, lb, ub, c, N, tv, kw):
        z, status = batched.mpc_box(A, B, Q, R, Qf, N, x0, lb, ub, c, tv=tv, **kw)
        ctx.mark_non_differentiable(status)
        _stash(ctx, (A, B, Q, R, Qf, x0, z, status), (lb, ub, c))
        ctx.N, ctx.tv = N, tv
        return z, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _gstatus):
        A, B, Q, R, Qf, x0, z, status, lb, ub, c = _recover(ctx, 8)
        need = ctx.needs_input_grad  # A, B, Q, R, Qf, x0, lb, ub, c
        batch = z.shape[0]
        H = batched.condense(A, B, Q, R, Qf, ctx.N, x0=x0, c=c, tv=ctx.tv, outputs=("H",))["H"]
        # dL/dH per instance, also where one H serves the batch: the instances'
        # x0 differ, and with them what condense_vjp makes of gf
        r = batched.solve_box_vjp(H.expand(batch, -1), z, lb, ub, gz.to(z.dtype), status=status,
                                  need_H=True)
        names = ("gA", "gB", "gQ", "gR", "gQf", "gx0", None, None, "gc")
        want = tuple(k for k, nd in zip(names, need) if nd and k)
        g = _cdiff.condense_vjp(A, B, Q, R, Qf, ctx.N, x0, c, tv=ctx.tv, gH=r["gH"], gf=r["gf"],
                                need=want) if want else {}
        glb, gub = _bound_grad(r["glb"], lb, need[6]), _bound_grad(r["gub"], ub, need[7])
        return (*(g.get(k) for k in names[:6]), glb, gub, g.get("gc"), None, None, None)


def mpc_box_model_diff(A, B, Q, R, Qf, N, x0, lb=None, ub=None, c=None, *, tv=False, **kw):
    """``batched.mpc_box`` (the fused condense + box-QP kernel) with gradients
    of the model as well: returns ``(z, status)``, bit for bit those of
    ``mpc_box``, where z carries the graph to A, B, c, Q, R, Qf, x0 and tensor
    lb / ub.  The backward pass condenses the instances (``batched.condense``),
    runs the box adjoint for d = dL/df, nu and dL/dH = d z'
    (``batched.solve_box_vjp``), and one launch of ``condense_vjp(gH, gf=d)``
    maps those to the inputs.  Conventions of ``mpc_box_diff`` and
    ``condense_diff``.  nx <= 4, nu <= 2, N * nu <= 32."""
    A, B, Q, R, Qf = _plant_tensors(A, B, Q, R, Qf)
    if _needs(A, B, Q, R, Qf, x0, lb, ub, c):
        _model_limits("mpc_box_model_diff", int(B.shape[-2]), int(B.shape[-1]),
                      int(N) * int(B.shape[-1]))
    return _MpcBoxModel.apply(A, B, Q, R, Qf, x0, lb, ub, c, int(N), bool(tv), kw)


def mpc_box_loop_model_diff(A, B, Q, R, Qf, N, x0, lb=None, ub=None, *, steps, plant=None, w=None,
                            x_ref=None, u_ref=None, cold=False, max_iter=0, tol=0.0):
    """``batched.mpc_box_loop`` (the one-launch input-box MPC episode) with
    gradients of the prediction model: returns ``(xs, us, zs, status)``, bit for
    bit the values of ``mpc_box_loop(..., plans=True)``.  H and F come from
    ``condense_diff`` on the model (A, B) and carry the graph to A, B, Q, R, Qf;
    the episode is ``box_loop_diff`` on the simulated plant, ``plant = (Ap, Bp)``,
    or on (A, B) itself when ``plant`` is None -- the gradient of A (and B) is then
    the sum of the model's part, through H and F, and the simulated plant's.
    Gradients also reach x0, tensor lb / ub, w and u_ref.  ``x_ref`` enters the
    linear term through Gam, whose gradient ``condense_vjp`` does not take:
    with it this raises NotImplementedError (``mpc_box_loop_diff`` tracks a state
    reference with a detached model).  nx <= 4, nu <= 2, N * nu <= 32."""
    if x_ref is not None:
        raise NotImplementedError(
            "mpc_box_loop_model_diff: x_ref together with gradients of the model is not "
            "implemented (its linear term runs through Gam); use mpc_box_loop_diff with A and B "
            "detached")
    A, B, Q, R, Qf = _plant_tensors(A, B, Q, R, Qf)
    N, T = int(N), int(steps)
    nx, nu = int(B.shape[-2]), int(B.shape[-1])
    _model_limits("mpc_box_loop_model_diff", nx, nu, N * nu)
    g = None
    if u_ref is None:
        H, F = _Condense.apply(A, B, Q, R, Qf, None, None, N, False, ("H", "F"))
    else:
        # the condensing call of mpc_box_loop with a reference: Gam comes along
        H, F, Gam = _Condense.apply(A, B, Q, R, Qf, None, None, N, False, ("H", "F", "Gam"))
        if Gam.shape[0] == 1:
            Gam = Gam[0]
        Rs = R.detach() + (_sym(R) - _sym(R).detach()) if _needs(R) else R
        g = batched.tracking_terms({"Gam": Gam}, Q.detach(), Rs, Qf.detach(), N, T, None, u_ref)
    Ap, Bp = (A, B) if plant is None else plant
    return box_loop_diff(H, F, Ap, Bp, x0, lb, ub, steps=T, g=g, w=w, cold=cold, max_iter=max_iter,
                         tol=tol)


# ------------------------------------------------ the polytope QP
def _batch_grad(g, ref):
    """The per-instance gradient ``g`` (b, w) for the operand ``ref``: summed
    over the batch where ``ref`` is shared ((w,))."""
    return g if ref.ndim == 2 else g.sum(0)


class _PolySolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, G, F, x0, f, hl, hu, lbz, ubz, qp, kw):
        if qp is None:
            qp = batched.PolyQP(H, G, F, lbz, ubz)
        z, y, status = qp.solve(x0, f, hl, hu, **kw)
        ctx.mark_non_differentiable(status)
        ctx.set_materialize_grads(False)
        _stash(ctx, (z, y, status), (x0, f, hl, hu, lbz, ubz))
        ctx.qp = qp
        return z, y, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gy, _gstatus):
        z, y, status, x0, f, hl, hu, lbz, ubz = _recover(ctx, 3)
        qp = ctx.qp
        need = ctx.needs_input_grad  # H, G, F, x0, f, hl, hu, lbz, ubz
        m = qp.m
        dt = z.dtype
        want = ["gf", "ghl", "ghu"] + (["gx0"] if need[3] else [])
        r = _pdiff.poly_solve_vjp(qp, y, None if gz is None else gz.to(dt),
                                  None if gy is None else gy.to(dt), status=status, need=want)
        names = ("gH", "gG", "gF", None, None, None, None, "glbz", "gubz")
        shared = tuple(k for k, nd in zip(names, need) if k and nd)
        s = _pdiff.shared_grads(qp, x0, z, y, r["gf"], r["e"], r["vstatus"],
                                need=shared) if shared else {}
        gH, gG, gF = (s.get(k) if nd else None for k, nd in zip(names[:3], need[:3]))
        gx0 = _batch_grad(r["gx0"], x0) if need[3] else None
        gf = _batch_grad(r["gf"], f) if need[4] else None
        ghl = _batch_grad(r["ghl"][:, :m], hl) if need[5] else None
        ghu = _batch_grad(r["ghu"][:, :m], hu) if need[6] else None
        glbz = _bound_grad(s.get("glbz"), lbz, need[7])
        gubz = _bound_grad(s.get("gubz"), ubz, need[8])
        return gH, gG, gF, gx0, gf, ghl, ghu, glbz, gubz, None, None


def poly_solve_diff(H, G, F, x0=None, f=None, hl=None, hu=None, lbz=None, ubz=None, *, qp=None,
                    **kw):
    """``batched.PolyQP(H, G, F, lbz, ubz).solve(x0, f, hl, hu)`` with
    gradients: returns ``(z, y, status)``, bit for bit the values of
    ``PolyQP.solve``, where z and y carry the graph to x0, f, hl, hu (per
    instance, or shared: summed over the batch), tensor lbz / ubz
    (Python-scalar bounds get none), packed H, G and F; status is
    non-differentiable.  The backward pass is ``poly_diff.poly_solve_vjp`` and,
    for the operands the batch shares, ``poly_diff.shared_grads``.  An instance
    whose forward did not end OPTIMAL (or whose adjoint meets a NaN or
    dependent active rows) contributes exact zeros to every gradient.
    ``qp``: a ``PolyQP`` the caller built from the same H, G, F, lbz and ubz;
    it skips the setup (the shared inverse and products) of every call, and the
    gradients still go to the tensors passed here.  Keyword arguments
    (max_iter, tol) go to ``solve``."""
    return _PolySolve.apply(H, G, F, x0, f, hl, hu, lbz, ubz, qp, kw)


def _mpc_poly_setup(who, refusal, A, B, Q, R, Qf, N, xlo, xhi, lb, ub):
    """What ``mpc_poly_diff`` and ``mpc_poly_loop_diff`` do first: refuse A or B
    that require grad (``refusal``: the caller's message), condense the shared
    model once -- through ``_Condense`` when a weight requires grad, so that
    H and F carry the graph to Q, R, Qf -- and tile the stage bounds over the
    horizon.  Returns ``(dt, dev, A, B, (Q, R, Qf), (H, F, Gam, Phi), (hl, hu,
    lbz, ubz))``; the weights are tensors (R a matrix) where they require grad,
    as given otherwise."""
    if _needs(A, B):
        raise NotImplementedError(refusal)
    dt, dev = batched._dt_dev(A)
    A, B = batched._dev(A, dt, dev), batched._dev(B, dt, dev)
    if A.ndim != 2 or B.ndim != 2:
        raise ValueError(f"{who}: the model (A, B) is shared by the batch")
    nx, nu = int(B.shape[0]), int(B.shape[1])
    outputs = ("H", "F", "Gam", "Phi")
    if _needs(Q, R, Qf):
        _model_limits(who, nx, nu, N * nu)
        A_, B_, Q, R, Qf = _plant_tensors(A, B, Q, R, Qf)
        cd = _Condense.apply(A_, B_, Q, R, Qf, None, None, N, False, outputs)
    else:
        cd = tuple(batched.condense(A, B, Q, R, Qf, N, outputs=outputs)[k] for k in outputs)
    bounds = tuple(batched._stage_bound(v, width, N, dt, dev, name) for v, width, name in (
        (xlo, nx, "xlo"), (xhi, nx, "xhi"), (lb, nu, "lb"), (ub, nu, "ub")))
    return dt, dev, A, B, (Q, R, Qf), tuple(v[0] for v in cd), bounds


def mpc_poly_diff(A, B, Q, R, Qf, N, x0, xlo=None, xhi=None, lb=None, ub=None, **kw):
    """One step of the linear MPC with a state box on x_1..x_N and an input
    box (the problem ``batched.mpc_poly_loop`` solves at every step), with
    gradients: returns ``(z, y, status)`` of the condensed QP, where z (b, N*nu)
    and y (b, rows) carry the graph to x0 (b, nx), xlo / xhi (scalar, (nx,) or
    (N*nx,)), lb / ub (scalar, (nu,) or (N*nu,)) given as tensors, and to the
    shared weights Q, R, Qf.  The shared model (A, B) is condensed once, as
    ``mpc_poly_loop`` does (H, F, Gam, Phi); the rows are xlo - Phi x0 <= Gam z
    <= xhi - Phi x0, taken as torch expressions, so that autograd carries their
    part of dL/dx0, and ``poly_solve_diff`` does the rest.  The weights'
    gradients come from one batch-1 call of ``condense_diff.condense_vjp`` on
    dL/dH and dL/dF -- exact, since Gam and Phi do not depend on the weights --
    within that adjoint's limits nx <= 4, nu <= 2, N * nu <= 32: outside them
    weights that require grad raise NotImplementedError.  So do A or B that
    require grad: their gradient needs dL/dGam and dL/dPhi, which
    ``condense_vjp`` does not take."""
    dt, dev, A, B, _, (H, F, Gam, Phi), (hl, hu, lbz, ubz) = _mpc_poly_setup(
        "mpc_poly_diff",
        "mpc_poly_diff: gradients through A and B need dL/dGam and dL/dPhi, which the "
        "adjoint of condensing does not take; detach them",
        A, B, Q, R, Qf, int(N), xlo, xhi, lb, ub)
    x0 = torch.as_tensor(x0, dtype=dt, device=dev)
    if x0.ndim != 2:
        raise ValueError(f"mpc_poly_diff: x0 must be (batch, {B.shape[0]}), got {tuple(x0.shape)}")
    rows = hl is not None or hu is not None
    free = x0 @ Phi.transpose(0, 1)
    hl, hu = (None if h is None else h[None, :] - free for h in (hl, hu))
    return poly_solve_diff(H, Gam if rows else None, F, x0, None, hl, hu, lbz, ubz, **kw)


# ------------------------------------------------ the one-launch polytope loop
def _step_grad(g, ref):
    """The per-step, per-instance gradient ``g`` (T, b, w) for the operand
    ``ref``: summed over the batch where ``ref`` is shared ((T, w))."""
    return g if ref.ndim == 3 else g.sum(1)


class _PolyLoop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, G, F, A, B, x0, hl, hu, lbz, ubz, E, w, g, e, steps, qp, kw):
        if qp is None:
            qp = batched.PolyQP(H, G, F, lbz, ubz)
        o = qp.loop(A, B, x0, steps, hl, hu, E, w, plans=True, multipliers=True, g=g, e=e, **kw)
        xs, us, zs, ys, status = o["xs"], o["us"], o["zs"], o["ys"], o["status"]
        ctx.mark_non_differentiable(status)
        ctx.set_materialize_grads(False)
        _stash(ctx, (A, B, xs, us, zs, ys, status), (hl, hu, lbz, ubz, E, g, e))
        ctx.qp = qp
        return xs, us, zs, ys, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gxs, gus, gzs, gys, _gstatus):
        A, B, xs, us, zs, ys, status, hl, hu, lbz, ubz, E, g, e = _recover(ctx, 7)
        qp = ctx.qp
        # H, G, F, A, B, x0, hl, hu, lbz, ubz, E, w, g, e
        nH, nG, nF, nA, nB, nx0, nhl, nhu, nlb, nub, nE, nw, ng, ne = ctx.needs_input_grad[:14]
        m, dt = qp.m, zs.dtype
        want = [k for k, nd in (("gx0", nx0), ("ghl", nhl or nlb), ("ghu", nhu or nub),
                                ("geps", nG or nE or ne), ("gf", nH or nG or nF or ng),
                                ("gw", nA or nB or nw)) if nd]
        r = _pdiff.poly_loop_vjp(qp, A, B, ys,
                                 *(None if t is None else t.to(dt) for t in (gxs, gus, gzs, gys)),
                                 E=E, status=status, need=want)
        shared = tuple(k for k, nd in (("gH", nH), ("gG", nG), ("gF", nF), ("gA", nA), ("gB", nB),
                                       ("gE", nE)) if nd)
        s = _pdiff.loop_shared_grads(qp, xs, us, zs, ys, r["gf"], r["geps"], r["gw"], r["vstatus"],
                                     need=shared) if shared else {}
        ghl = _batch_grad(r["ghl"][:, :m], hl) if nhl else None
        ghu = _batch_grad(r["ghu"][:, :m], hu) if nhu else None
        glbz = _bound_grad(r["ghl"][:, m:].sum(0), lbz, True) if nlb else None
        gubz = _bound_grad(r["ghu"][:, m:].sum(0), ubz, True) if nub else None
        gg = _step_grad(r["gf"], g) if ng else None
        ge = _step_grad(-r["geps"][:, :, :m], e) if ne else None
        return (s.get("gH"), s.get("gG"), s.get("gF"), s.get("gA"), s.get("gB"),
                r["gx0"] if nx0 else None, ghl, ghu, glbz, gubz, s.get("gE"),
                r["gw"] if nw else None, gg, ge, None, None, None)


def poly_loop_diff(H, G, F, A, B, x0, hl=None, hu=None, lbz=None, ubz=None, *, steps, E=None,
                   w=None, g=None, e=None, cold=False, max_iter=0, tol=0.0, qp=None):
    """``batched.PolyQP(H, G, F, lbz, ubz).loop(A, B, x0, steps, hl, hu, E, w,
    g=g, e=e, plans=True, multipliers=True)`` with gradients: returns ``(xs, us,
    zs, ys, status)``, bit for bit the values of ``PolyQP.loop``, where xs (T+1,
    b, nx), us (T, b, nu), zs (T, b, n) and ys (T, b, m_total) carry the graph
    to x0 (b, nx), hl, hu ((m,) shared: summed over the batch, or (b, m)), g
    ((T, n) or (T, b, n)), e ((T, m) or (T, b, m)), w (T, b, nx), tensor lbz /
    ubz (Python-scalar bounds get none), packed H, G, F, E and the plant's A, B;
    status is non-differentiable.  The backward pass is one launch of
    ``poly_diff.poly_loop_vjp`` (after one product launch when the loss reads
    zs) and, for the operands the episode shares, ``poly_diff.loop_shared_grads``.
    An instance with a step that did not end OPTIMAL (or whose adjoint meets a
    NaN or dependent active rows) contributes exact zeros to every gradient.
    ``qp``: a ``PolyQP`` the caller built from the same H, G, F, lbz and ubz; it
    skips the setup, and the gradients still go to the tensors passed here.
    The soft loop has no adjoint: ``soft=`` is not accepted."""
    kw = dict(cold=bool(cold), max_iter=int(max_iter), tol=float(tol))
    return _PolyLoop.apply(H, G, F, A, B, x0, hl, hu, lbz, ubz, E, w, g, e, int(steps), qp, kw)


def mpc_poly_loop_diff(A, B, Q, R, Qf, N, x0, xlo=None, xhi=None, lb=None, ub=None, *, steps,
                       plant=None, w=None, x_ref=None, u_ref=None, cold=False, max_iter=0,
                       tol=0.0):
    """``batched.mpc_poly_loop`` (the one-launch episode of the linear MPC with
    a state box on x_1..x_N and an input box) with gradients: returns ``(xs,
    us, zs, ys, status)``, bit for bit the values of ``mpc_poly_loop(...,
    plans=True, multipliers=True)``.  The ``PolyQP`` is built as there (the
    shared model condensed once; G = Gam, E = Phi, the state box tiled over the
    horizon) and ``poly_loop_diff`` runs the episode: gradients reach x0, xlo /
    xhi (scalar, (nx,) or (N*nx,)) and lb / ub (scalar, (nu,) or (N*nu,)) given
    as tensors, w, the references x_ref / u_ref (through
    ``batched.tracking_terms``) and the simulated plant ``plant = (A_p, B_p)``.
    The shared weights Q, R, Qf get theirs from one batch-1 call of
    ``condense_diff.condense_vjp`` on dL/dH and dL/dF (exact: Gam and Phi do not
    depend on them) plus, with a reference, the tracking term's, within the
    limits nx <= 4, nu <= 2, N * nu <= 32: outside them weights that require grad
    raise NotImplementedError.  So do a model A or B that require grad: their
    gradient needs dL/dGam and dL/dPhi, which ``condense_vjp`` does not take."""
    N, T = int(N), int(steps)
    dt, dev, A, B, (Q, R, Qf), (H, F, Gam, Phi), (hl, hu, lbz, ubz) = _mpc_poly_setup(
        "mpc_poly_loop_diff",
        "mpc_poly_loop_diff: gradients through the model's A and B need dL/dGam and dL/dPhi, "
        "which the adjoint of condensing does not take; detach them (plant=(A_p, B_p) is "
        "differentiated)", A, B, Q, R, Qf, N, xlo, xhi, lb, ub)
    rows = hl is not None or hu is not None
    g = None
    if x_ref is not None or u_ref is not None:
        g = batched.tracking_terms({"Gam": Gam}, *(batched._dev(v, dt, dev) for v in (Q, R, Qf)),
                                   N, T, x_ref, u_ref)
    Ap, Bp = (A, B) if plant is None else plant
    return poly_loop_diff(H, Gam if rows else None, F, Ap, Bp, x0, hl, hu, lbz, ubz, steps=T,
                          E=Phi if rows else None, w=w, g=g, cold=cold, max_iter=max_iter, tol=tol)
