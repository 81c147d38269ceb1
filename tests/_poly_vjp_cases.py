"""Shared by tests/test_poly_vjp_host.py and tests/test_gpu_poly_vjp.py: the
NumPy closed form of the polytope-QP adjoint (include/mpcqp_poly_diff.h) and
the problems it is checked on, which are those of tests/_poly_cases.py
(family_a, family_b, maxiter_case) plus one shape with n > 64.

At the optimum of  min 1/2 z'Hz + (F x0 + f1)'z,  lo <= C z <= hi,  C = [G; I],
with the signed multipliers y (> 0 at the upper side) the active set is taken
from the given y, A = {i : y_i != 0}.  With gz = dL/dz, gy = dL/dy,
Ut = C H^-1 and M = Ut C':

    q = H^-1 gz,  r = Ut gz,  e_A = M_AA^-1 (r_A - gy_A),  e = 0 elsewhere
    gf = dL/df1 = -(q - Ut_A' e_A),   gx0 = F' gf
    ghu_i = e_i (y_i > 0),  ghl_i = e_i (y_i < 0)          (all m_total rows)
    dL/dH = gf z' (packed (i, j<i): S_ij + S_ji, (i, i): S_ii),  dL/dF = gf x0',
    dL/dG = rows < m of (y gf' - e z')
"""
import numpy as np

from _poly_cases import INF, Case, family_a, family_b, maxiter_case  # noqa: F401
from _poly_loop_cases import cached


def pack_lower(H):
    r, c = np.tril_indices(H.shape[-1])
    return np.ascontiguousarray(H[..., r, c])


def unpack_lower(P, n):
    H = np.zeros((n, n))
    r, c = np.tril_indices(n)
    H[r, c] = P
    return H + np.tril(H, -1).T


def closed_form(H, C, m, F, x0, z, y, gz, gy):
    """dict(gf, gx0, ghl, ghu, e, gH (packed, folded), gF, gG) of one instance;
    C (m_total, n) = [G; I], F (n, nx) or None, x0 (nx,) or None."""
    n = H.shape[0]
    Hinv = np.linalg.inv(H)
    Ut = C @ Hinv
    M = Ut @ C.T
    act = y != 0
    q, r = Hinv @ gz, Ut @ gz
    e = np.zeros(C.shape[0])
    if act.any():
        e[act] = np.linalg.solve(M[np.ix_(act, act)], r[act] - gy[act])
    gf = -(q - Ut[act].T @ e[act])
    S = np.outer(gf, z)
    GH = S + S.T
    GH[np.diag_indices(n)] = np.diag(S)
    out = dict(gf=gf, e=e, ghl=np.where(y < 0, e, 0.0), ghu=np.where(y > 0, e, 0.0),
               gH=pack_lower(GH), gG=(np.outer(y, gf) - np.outer(e, z))[:m])
    if F is not None:
        out["gx0"] = F.T @ gf
        out["gF"] = np.outer(gf, np.zeros(F.shape[1]) if x0 is None else x0)
    return out


def of_case(case, i, z, y, gz, gy):
    """closed_form for instance i of a _poly_cases.Case at the given (z, y)."""
    x0 = None if case.x0 is None else case.x0[i]
    return closed_form(case.H, case.qp.Call, case.m, case.F, x0, z, y, gz, gy)


def upstream(case, seed=0):
    """Fixed random (gz (b, n), gy (b, m_total)) for a case."""
    rng = np.random.default_rng(7000 + 100 * case.n + case.mt + seed)
    return rng.standard_normal((case.batch, case.n)), rng.standard_normal((case.batch, case.mt))


# ------------------------------------------------------------ n > 64
# (n, m) = (130, 40), no box, nx = 16: three trips of the kernel's 64-lane loop
# over z, the last partial; nx at its limit; gz wider than a wavefront.
# WIDE_SCALE multiplies x0 and f1 as SCALE_A does in _poly_cases: of the grid
# 0.25 .. 1.5 the value at which the oracle's active sets are best separated
# (3.6e-3 of the scale; 10 to 17 active rows per instance, both sides).
WIDE_SHAPE, WIDE_NX, WIDE_BATCH, WIDE_SCALE = (130, 40), 16, 6, 0.35
SEPARATION = 1e-3  # active sets are separated by this much (times the scale)


def wide_case(fp32=False):
    """family_a's recipe at (130, 40) without the box: random SPD H, rows of
    unit expected norm, -h1 <= G z <= h2 with h ~ U(0.2, 1)."""
    def make():
        n, m = WIDE_SHAPE
        rng = np.random.default_rng(1000 * n + m)
        M = rng.normal(size=(n, n))
        H = M @ M.T / n + 0.5 * np.eye(n)
        G = rng.normal(size=(m, n)) / np.sqrt(n)
        F = rng.normal(size=(n, WIDE_NX)) / np.sqrt(WIDE_NX)
        x0 = rng.normal(size=(WIDE_BATCH, WIDE_NX)) * WIDE_SCALE
        f1 = rng.normal(size=(WIDE_BATCH, n)) * WIDE_SCALE
        hl = -rng.uniform(0.2, 1.0, size=(WIDE_BATCH, m))
        hu = rng.uniform(0.2, 1.0, size=(WIDE_BATCH, m))
        return Case(H, G, F, None, None, x0, f1, hl, hu, fp32)
    return cached(("polyWide", fp32), make)
