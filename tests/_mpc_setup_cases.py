"""The cases of test_gpu_mpc_box_setup.py: plants and weights, and the oracle
reference of a case, computed once and shared between the tests that need it."""
import functools

import numpy as np

from oracle import condense as oc
from oracle import qp as oq
from oracle import session1 as s1


def plants(rng, nx, nu, N, tv, batch=None):
    """Random (marginally) stable plants and weights, Qf = 3 Q, drawn as
    test_gpu_mpc_box_rows.py draws them; batch=None gives one instance."""
    lead = () if batch is None else (batch,)
    shA = lead + ((N, nx, nx) if tv else (nx, nx))
    shB = lead + ((N, nx, nu) if tv else (nx, nu))
    A = rng.normal(size=shA) * (0.8 / np.sqrt(nx)) + 0.4 * np.eye(nx)
    rho = np.abs(np.linalg.eigvals(A.reshape(-1, nx, nx))).max(axis=-1).reshape(A.shape[:-2])
    A = A / np.maximum(1.0, rho / 1.02)[..., None, None]
    B = rng.normal(size=shB)
    M = rng.normal(size=(nx, nx))
    Q = M @ M.T / nx + 0.2 * np.eye(nx)
    R = np.diag(rng.uniform(0.1, 1.0, nu))
    return A, B, Q, R, 3 * Q


def cfg2_plant():
    A, B, Q, R, Pf, _ = s1.fhc_setup()
    return A, B, Q, R.reshape(1, 1), Pf


def case(seed, nx, nu, N, tv, drift, batch):
    """Inputs of one case; nx = 0 stands for the config-2 plant (n = N, |u| <= 1,
    x0 ~ U(-10, 10)^2)."""
    rng = np.random.default_rng(seed)
    if nx == 0:
        A, B, Q, R, Qf = cfg2_plant()
        A = np.broadcast_to(A, (batch, 2, 2)).copy()
        B = np.broadcast_to(B, (batch, 2, 1)).copy()
        x0 = rng.uniform(-10, 10, (batch, 2))
        nx, n = 2, N
        lb, ub = -np.ones((batch, n)), np.ones((batch, n))
    else:
        A, B, Q, R, Qf = plants(rng, nx, nu, N, tv, batch)
        x0 = rng.normal(size=(batch, nx)) * 3
        n = N * nu
        lb = -rng.uniform(0.2, 1.0, (batch, n))
        ub = rng.uniform(0.2, 1.0, (batch, n))
    c = rng.normal(size=(batch, N, nx)) * 0.3 if drift else None
    return A, B, Q, R, Qf, x0, lb, ub, c


def reference(A, B, Q, R, Qf, N, x0, lb, ub, c):
    """Explicit condensing + active set per instance: (z_ref (b, n), cond(H) (b,))."""
    zs, conds = [], []
    for b in range(x0.shape[0]):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b], c=None if c is None else c[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], lb[b], ub[b])
        zs.append(zr)
        conds.append(np.linalg.cond(ref["H"]))
    return np.stack(zs), np.array(conds)


@functools.lru_cache(maxsize=None)
def case_with_reference(seed, nx, nu, N, tv, drift, batch, x0_scale=1.0, c_scale=1.0):
    """The case and its reference, computed once; the scales shrink x0 and the
    drift (the fp32 runs of the config-2 plant: 0.3 and 0.1, as test_rows_fp32
    does).  The arrays are shared between tests: read only."""
    A, B, Q, R, Qf, x0, lb, ub, c = case(seed, nx, nu, N, tv, drift, batch)
    x0 = x0 * x0_scale
    if c is not None:
        c = c * c_scale
    zr, cond = reference(A, B, Q, R, Qf, N, x0, lb, ub, c)
    for a in (A, B, Q, R, Qf, x0, lb, ub, zr, cond) + (() if c is None else (c,)):
        a.setflags(write=False)
    return (A, B, Q, R, Qf, x0, lb, ub, c), zr, cond
