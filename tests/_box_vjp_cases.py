"""Shared by tests/test_box_vjp_host.py and tests/test_gpu_box_vjp.py: the
NumPy closed form of the box-QP adjoint and the problems it is checked on.

At the optimum z of  min 1/2 z'Hz + f'z, lb <= z <= ub  with A the rows at a
bound (exact comparison) and F the free rows, for g = dL/dz:

    d_F  = -H_FF^-1 g_F, d_A = 0          dL/df = d
    nu_A = g_A + H_AF d_F                 dL/dlb_i = nu_i at lb_i, dL/dub_i = nu_i at ub_i
    dL/dH = d z' (unsymmetrised)          packed (i, j<i): d_i z_j + d_j z_i, (i, i): d_i z_i

and for the condensed MPC step (H = Gam' Qhat Gam + Rhat, f = Gam' Qhat xbar,
xbar = Phi x0 + w), with dX = Gam d and X = xbar + Gam z by stages:

    dL/dx0 = F'd,  dL/dQ = sym(sum_{k<N-1} dX_k X_k'),  dL/dQf = sym(dX_{N-1} X_{N-1}'),
    dL/dR = sym(sum_k d_k z_k').
"""
import functools

import numpy as np

from oracle import condense as oc
from oracle import qp as oq
from oracle import session1 as s1

MARGIN = 1e-3  # a case is non-degenerate above this (multipliers and free-row slack)
SIZES = (1, 5, 17, 20, 32)  # N * nu of the session-1 cases (nu = 1)
COUNT = 32


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def pack_lower(H):
    n = H.shape[-1]
    r, c = np.tril_indices(n)
    return np.ascontiguousarray(H[..., r, c])


def active_sets(z, lb, ub):
    at_lb = z == lb
    at_ub = (z == ub) & ~at_lb
    return at_lb, at_ub


def closed_form(H, z, lb, ub, g):
    """dict(d, nu, glb, gub, gH (packed)) for one instance (dense H)."""
    n = z.size
    lb = np.broadcast_to(-np.inf if lb is None else lb, (n,))
    ub = np.broadcast_to(np.inf if ub is None else ub, (n,))
    at_lb, at_ub = active_sets(z, lb, ub)
    A = at_lb | at_ub
    F = ~A
    d = np.zeros(n)
    if F.any():
        d[F] = -np.linalg.solve(H[np.ix_(F, F)], g[F])
    nu = np.zeros(n)
    nu[A] = g[A] + H[np.ix_(A, F)] @ d[F]
    G = np.outer(d, z)
    GH = G + G.T
    GH[np.diag_indices(n)] = np.diag(G)
    return dict(d=d, nu=nu, glb=np.where(at_lb, nu, 0.0), gub=np.where(at_ub, nu, 0.0),
                gH=pack_lower(GH))


def mpc_grads(cd, z, d, N, nx, nu):
    """dict(x0, Q, Qf, R) from the condensed matrices of one instance."""
    dX = (cd["Gam"] @ d).reshape(N, nx)
    X = (cd["xbar"] + cd["Gam"] @ z).reshape(N, nx)
    return dict(x0=cd["F"].T @ d, Q=sym(dX[:-1].T @ X[:-1]), Qf=sym(np.outer(dX[-1], X[-1])),
                R=sym(d.reshape(N, nu).T @ z.reshape(N, nu)))


def margin(H, f, lb, ub, z):
    """Smallest active multiplier / smallest slack of a free row."""
    at_lb, at_ub = active_sets(z, lb, ub)
    kkt = H @ z + f
    vals = [np.inf]
    if at_lb.any():
        vals.append(kkt[at_lb].min())
    if at_ub.any():
        vals.append((-kkt[at_ub]).min())
    F = ~(at_lb | at_ub)
    if F.any():
        vals.append(np.minimum(z[F] - lb[F], ub[F] - z[F]).min())
    return float(min(vals))


def _finish(p):
    """Oracle solutions, margins and a fixed loss direction g (L = g.z)."""
    b, n = p["x0"].shape[0], p["N"] * p["nu"]
    p["n"] = n
    p["cd"] = [oc.condense(p["A"], p["B"], p["Q"], p["R"], p["Qf"], p["N"], x0=p["x0"][i])
               for i in range(b)]
    p["H"] = np.stack([c["H"] for c in p["cd"]])
    p["f"] = np.stack([c["f"] for c in p["cd"]])
    p["z"] = np.stack([oq.box_qp(p["H"][i], p["f"][i], p["lb"][i], p["ub"][i])[0]
                       for i in range(b)])
    p["margin"] = np.array([margin(p["H"][i], p["f"][i], p["lb"][i], p["ub"][i], p["z"][i])
                            for i in range(b)])
    p["nondeg"] = p["margin"] > MARGIN
    p["g"] = np.random.default_rng(1000 + n).standard_normal((b, n))
    return p


@functools.lru_cache(maxsize=None)
def session1_batch(n, count=COUNT, seed=11, spread=10.0):
    """The session-1 plant (nx = 2, nu = 1, N = n), x0 ~ U(-spread, spread)^2,
    |u| <= 1.  (At spread = 10 most instances of a long horizon saturate every
    row; the kernel tests also use a smaller spread for mixed active sets.)"""
    A, B, Q, R, Pf, _ = s1.fhc_setup()
    rng = np.random.default_rng(seed + n)
    return _finish(dict(A=A, B=B, Q=Q, R=R.reshape(1, 1), Qf=Pf, N=n, nx=2, nu=1,
                        x0=rng.uniform(-spread, spread, (count, 2)), lb=-np.ones((count, n)),
                        ub=np.ones((count, n))))


@functools.lru_cache(maxsize=None)
def random_batch(nx=3, nu=2, N=4, count=COUNT, seed=23, box=0.4):
    """A random plant with |u| <= box, one x0 ~ N(0, 1) per instance."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, nx))
    A *= 0.95 / np.abs(np.linalg.eigvals(A)).max()
    B = rng.standard_normal((nx, nu))
    spd = lambda k: (lambda M: M @ M.T / k + 0.5 * np.eye(k))(rng.standard_normal((k, k)))  # noqa: E731
    Q, R, Qf = spd(nx), spd(nu), spd(nx)
    n = N * nu
    return _finish(dict(A=A, B=B, Q=Q, R=R, Qf=Qf, N=N, nx=nx, nu=nu,
                        x0=rng.standard_normal((count, nx)), lb=-box * np.ones((count, n)),
                        ub=box * np.ones((count, n))))


def nondegenerate(p, count):
    """Indices of the first ``count`` non-degenerate instances of a batch."""
    idx = np.nonzero(p["nondeg"])[0][:count]
    assert idx.size == count, (idx.size, count)
    return idx
