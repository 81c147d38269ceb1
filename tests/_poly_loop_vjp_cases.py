"""Shared by tests/test_poly_loop_vjp_host.py and tests/test_gpu_poly_loop_vjp.py:
the NumPy restatement of the reverse-time adjoint of the one-launch polytope
MPC loop (include/mpcqp_poly_loop_diff.h) on top of the per-step closed form of
tests/_poly_vjp_cases.py, the oracle's episodes it is checked on (those of
tests/_poly_loop_cases.py, with multipliers), fixed random upstream gradients
and the separation of an episode's active sets.

Forward, per step:  z_t = argmin 1/2 z'Hz + (F x_t + g_t)'z  over
hl - E x_t - e_t <= G z <= hu - E x_t - e_t, lbz <= z <= ubz;  u_t = z_t[:nu],
x_{t+1} = A x_t + B u_t + w_t.  Backward, with the upstream gxs, gus, gzs, gys:

    lam = gxs[T]
    for t = T-1 .. 0:
        gz = gzs[t];  gz[:nu] += gus[t] + B'lam
        (gf_t, eps_t) = closed_form at (z_t, y_t) with (gz, gys[t])
        gw_t = lam;  ghl, ghu += eps_t on the side held
        lam = gxs[t] + A'lam + F'gf_t - E'eps_t[:m]
    gx0 = lam
"""
import numpy as np

import _poly_vjp_cases as pv


def episode(qp, x0, T, plant=None, w=None):
    """The oracle's closed loop with multipliers: xs (T+1, nx), zs (T, n), ys
    (T, mt).  Raises ValueError when a step's QP is empty."""
    A, B = (qp.A, qp.B) if plant is None else plant
    xs = np.zeros((T + 1, qp.nx))
    zs = np.zeros((T, qp.n))
    ys = np.zeros((T, qp.mt))
    xs[0] = x0
    for t in range(T):
        zs[t], ys[t], _ = qp.step(xs[t])
        xs[t + 1] = A @ xs[t] + B @ zs[t, :qp.nu] + (0.0 if w is None else w[t])
    return xs, zs, ys


def upstream(T, nx, nu, n, mt, seed=0, batch=None):
    """Fixed standard-normal (gxs (T+1, [b,] nx), gus (T, [b,] nu), gzs (T, [b,] n),
    gys (T, [b,] mt))."""
    rng = np.random.default_rng(9100 + 1000 * n + 10 * mt + T + seed)
    mid = () if batch is None else (batch,)
    return (rng.standard_normal((T + 1, *mid, nx)), rng.standard_normal((T, *mid, nu)),
            rng.standard_normal((T, *mid, n)), rng.standard_normal((T, *mid, mt)))


def loss(xs, zs, ys, nu, gxs, gus, gzs, gys):
    """The linear loss whose gradients the upstreams are."""
    return float((gxs * xs).sum() + (gus * zs[:, :nu]).sum() + (gzs * zs).sum() + (gys * ys).sum())


def recursion(qp, xs, zs, ys, gxs=None, gus=None, gzs=None, gys=None, plant=None):
    """The reverse-time recursion for one instance: dict of gx0 (nx), ghl, ghu
    (mt, summed over the steps), geps (T, mt), gf (T, n), gw (T, nx) and the
    shared operands' gH (packed, folded), gF, gG, gE, gA, gB."""
    A, B = (qp.A, qp.B) if plant is None else plant
    T, n, m, mt, nx, nu = zs.shape[0], qp.n, qp.m, qp.mt, qp.nx, qp.nu
    zero = lambda v, shape: np.zeros(shape) if v is None else v  # noqa: E731
    gxs, gus = zero(gxs, (T + 1, nx)), zero(gus, (T, nu))
    gzs, gys = zero(gzs, (T, n)), zero(gys, (T, mt))
    o = dict(ghl=np.zeros(mt), ghu=np.zeros(mt), geps=np.zeros((T, mt)), gf=np.zeros((T, n)),
             gw=np.zeros((T, nx)), gH=np.zeros(n * (n + 1) // 2), gF=np.zeros((n, nx)),
             gG=np.zeros((m, n)), gE=np.zeros((m, nx)), gA=np.zeros((nx, nx)),
             gB=np.zeros((nx, nu)))
    lam = gxs[T].copy()
    for t in range(T - 1, -1, -1):
        gz = gzs[t].copy()
        gz[:nu] += gus[t] + B.T @ lam
        cf = pv.closed_form(qp.H, qp.Call, m, qp.F, xs[t], zs[t], ys[t], gz, gys[t])
        o["gf"][t], o["geps"][t], o["gw"][t] = cf["gf"], cf["e"], lam
        o["ghl"] += cf["ghl"]
        o["ghu"] += cf["ghu"]
        o["gH"] += cf["gH"]
        o["gF"] += cf["gF"]
        o["gG"] += cf["gG"]
        o["gE"] -= np.outer(cf["e"][:m], xs[t])
        o["gA"] += np.outer(lam, xs[t])
        o["gB"] += np.outer(lam, zs[t, :nu])
        lam = gxs[t] + A.T @ lam + cf["gx0"]
        if qp.E is not None:
            lam = lam - qp.E.T @ cf["e"][:m]
    o["gx0"] = lam
    return o


def separation(qp, xs, zs, ys, e=None):
    """How far an episode's active sets are from changing: the minimum over the
    steps of |y| on the active rows and of the slack to the nearer bound on the
    inactive rows."""
    sep = np.inf
    for t in range(zs.shape[0]):
        lo, hi = qp.bounds(xs[t])
        if e is not None:
            lo[:qp.m] -= e[t]
            hi[:qp.m] -= e[t]
        cz = qp.Call @ zs[t]
        act = ys[t] != 0
        slack = np.minimum(cz - lo, hi - cz)
        sep = min(sep, np.abs(ys[t][act]).min(initial=np.inf), slack[~act].min(initial=np.inf))
    return float(sep)
