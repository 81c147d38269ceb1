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
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import batched

__all__ = ["solve_box_diff", "mpc_box_diff"]

MAX_N = batched.BOX_VJP_MAX_N


def _needs(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _like_input(g, ref):
    """The gradient ``g`` (shared: (n,), batched: (b, n)) in the shape of the
    bound tensor ``ref`` it belongs to (a 0-dim bound is spread over the rows)."""
    if ref.ndim == 0:
        return g.sum()
    return g.reshape(ref.shape)


class _SolveBox(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, f, lb, ub, kw):
        z, status = batched.solve_box(H, f, lb, ub, **kw)
        ctx.mark_non_differentiable(status)
        tens = [H, f, z, status]
        ctx.lb_t = isinstance(lb, torch.Tensor)
        ctx.ub_t = isinstance(ub, torch.Tensor)
        ctx.lb = None if ctx.lb_t else lb
        ctx.ub = None if ctx.ub_t else ub
        if ctx.lb_t:
            tens.append(lb)
        if ctx.ub_t:
            tens.append(ub)
        ctx.save_for_backward(*tens)
        return z, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _gstatus):
        saved = list(ctx.saved_tensors)
        H, f, z, status = saved[:4]
        rest = saved[4:]
        lb = rest.pop(0) if ctx.lb_t else ctx.lb
        ub = rest.pop(0) if ctx.ub_t else ctx.ub
        need = ctx.needs_input_grad
        r = batched.solve_box_vjp(H, z, lb, ub, gz.to(z.dtype), status=status, need_H=need[0])
        gH = r["gH"] if need[0] else None
        gf = None
        if need[1]:
            gf = r["gf"] if f.ndim == 2 else r["gf"].sum(0)
        glb = _like_input(r["glb"], lb) if ctx.lb_t and need[2] else None
        gub = _like_input(r["gub"], ub) if ctx.ub_t and need[3] else None
        return gH, gf, glb, gub, None


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
        tens = [A, B, Q, R, Qf, x0, z, status]
        ctx.flags = [isinstance(t, torch.Tensor) for t in (lb, ub, c)]
        ctx.plain = [None if isinstance(t, torch.Tensor) else t for t in (lb, ub, c)]
        tens += [t for t in (lb, ub, c) if isinstance(t, torch.Tensor)]
        ctx.save_for_backward(*tens)
        ctx.N, ctx.tv = N, tv
        return z, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _gstatus):
        saved = list(ctx.saved_tensors)
        A, B, Q, R, Qf, x0, z, status = saved[:8]
        rest = saved[8:]
        lb, ub, c = (rest.pop(0) if fl else pl for fl, pl in zip(ctx.flags, ctx.plain))
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
        glb = _like_input(r["glb"], lb) if ctx.flags[0] and need[6] else None
        gub = _like_input(r["gub"], ub) if ctx.flags[1] and need[7] else None
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
