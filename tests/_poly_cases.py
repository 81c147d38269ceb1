"""Scenarios and the oracle-side reference of the stand-alone polytope solver
(mpcqp_solve_poly / mpcqp_poly_setup + mpcqp_poly_solve, dual_range_kernel),
shared by tests/test_poly_host.py (reference only) and tests/test_gpu_poly.py.

Per instance the reference is oracle.qp.poly_qp on

    min 1/2 z'Hz + (F x0 + f1)'z   s.t.  hl <= G z <= hu,  lbz <= z <= ubz

with the rows stacked as C z <= d (finite sides only), certified by
oracle.qp.kkt_poly below 1e-9 * scale, and the multipliers folded back to the
signed y over [G; I] (> 0 at the upper bound, < 0 at the lower): all of that is
_poly_loop_cases.LoopQP.step, used here with the gradient map [F, I] and the
"state" [x0; f1], so that its F x is F x0 + f1.  (m = 0: oracle.qp.box_qp,
certified by oracle.qp.kkt_box.)

An fp32 case rounds every input to fp32 first and hands the rounded data to
the oracle as fp64.
"""
import numpy as np

from _poly_loop_cases import LoopQP, cached
from oracle import qp as oq

INF = np.inf


def f32(a):
    return None if a is None else np.asarray(a, np.float32).astype(np.float64)


class Case:
    """One batch of polytope QPs on shared H, G, F, lbz, ubz.  x0 (b, nx) and
    f1 (b, n) or None; hl, hu (b, m), (m,) or None.  ``ref`` = per instance
    (z, y, act) of the oracle; ``scale`` = per instance max(1, |bounds|, |f|)."""

    def __init__(self, H, G, F, lbz, ubz, x0, f1, hl, hu, fp32=False):
        if fp32:
            H, G, F, lbz, ubz, x0, f1, hl, hu = map(f32, (H, G, F, lbz, ubz, x0, f1, hl, hu))
        self.H, self.G, self.F, self.x0, self.f1, self.hl, self.hu = H, G, F, x0, f1, hl, hu
        self.n = n = H.shape[0]
        self.nx = 0 if F is None else F.shape[1]
        self.batch = b = (x0 if x0 is not None else f1).shape[0]
        Faug = np.eye(n) if F is None else np.hstack([F, np.eye(n)])
        self.qp = LoopQP(H, Faug, G, None, None, None, lbz, ubz, None, np.zeros((Faug.shape[1], 1)))
        self.m, self.mt, self.lbz, self.ubz = self.qp.m, self.qp.mt, lbz, ubz
        z1 = np.zeros((b, n)) if f1 is None else f1
        self.xaug = z1 if F is None else np.hstack([np.zeros((b, self.nx)) if x0 is None else x0, z1])
        self.f = self.xaug @ Faug.T                      # the gradients F x0 + f1
        self.ref = [self._solve(i) for i in range(b)]

    def rows(self, i):
        """(hl, hu) of instance i as full (m,) arrays (+-inf where absent)."""
        def one(h, fill):
            if h is None:
                return np.full(self.m, fill)
            return np.array(h if h.ndim == 1 else h[i], float)
        return one(self.hl, -INF), one(self.hu, INF)

    def bounds(self, i):
        """(lo, hi) of the m_total rows [G; I] of instance i."""
        return self.qp.bounds(self.xaug[i], *self.rows(i))

    def scale(self, i):
        lo, hi = self.bounds(i)
        fin = np.concatenate([lo[np.isfinite(lo)], hi[np.isfinite(hi)]])
        return max(1.0, np.abs(fin).max(initial=0.0), np.abs(self.f[i]).max(initial=0.0))

    def _solve(self, i):
        if self.m > 0:
            return self.qp.step(self.xaug[i], 0.0, *self.rows(i))
        lb, ub = self.qp.lbz, self.qp.ubz
        z, mult, _ = oq.box_qp(self.H, self.f[i], lb, ub)
        kkt = oq.kkt_box(self.H, self.f[i], lb, ub, z)
        assert kkt < 1e-9 * self.scale(i), kkt
        y = -mult                                        # box_qp: mult > 0 at the lower bound
        return z, y, np.where(y > 0, 2, np.where(y < 0, 1, 0))

    def slack(self, i):
        """Per row of [G; I] the distance of the oracle's C z to the nearer bound."""
        lo, hi = self.bounds(i)
        cz = self.qp.Call @ self.ref[i][0]
        return np.minimum(cz - lo, hi - cz)

    def separation(self, i):
        """min over the rows of |y| (active) or slack (inactive), over scale."""
        _, y, act = self.ref[i]
        return float(np.where(act > 0, np.abs(y), self.slack(i)).min()) / self.scale(i)

    def active_rank_ok(self, i):
        act = self.ref[i][2] > 0
        return act.sum() == 0 or np.linalg.matrix_rank(self.qp.Call[act]) == act.sum()


def check_kkt(case, i, z, y, stat_tol, row_tol):
    """KKT certificate of a device answer (z, y) of instance i, at the absolute
    tolerances stat_tol (a scalar) and row_tol (a scalar or one value per row
    of [G; I]): stationarity |H z + f + C'y| < stat_tol; feasibility of every
    row to row_tol; y > 0 only on rows within row_tol of their upper bound and
    y < 0 only within row_tol of their lower (sign and complementarity)."""
    qp = case.qp
    assert np.abs(qp.H @ z + case.f[i] + qp.Call.T @ y).max() < stat_tol
    lo, hi = case.bounds(i)
    cz = qp.Call @ z
    row_tol = np.broadcast_to(row_tol, cz.shape)
    assert (cz - hi < row_tol).all() and (lo - cz < row_tol).all()
    up, dn = y > 0, y < 0
    assert (np.abs(cz - hi)[up] < row_tol[up]).all() and (np.abs(cz - lo)[dn] < row_tol[dn]).all()


# ------------------------------------------------------------------ family A
# (n, m) with a box: m_total = m + n = 5, 16, 19, 32, 37, 48, 51, 64, one per
# dual_range_kernel<T, BS>, BS = ceil(m_total / 8) = 1..8: padded and unpadded
# sizes, m > n, and the limit 64.
SHAPES_A = [(3, 2), (6, 10), (8, 11), (12, 20), (10, 27), (20, 28), (24, 27), (24, 40)]
BATCH_A, NX_A = 6, 3
# x0 and f1 are normal draws times SCALE_A[(n, m)].  The scale decides how
# many rows are active: about n - 2 of them at 2, which is next to a vertex,
# where fp32 cannot tell the active set from its neighbours.  Per shape it is
# the value of the grid 0.5 .. 3 at which the oracle's active sets are best
# separated (smallest |y| of an active row or slack of an inactive one, over
# the batch), among those at which every instance has two or more active rows
# and the shape has rows at both sides and box rows.  The rows of G are scaled
# to unit expected norm (normal / sqrt(n)): with unscaled rows and m > n the
# rows alone hold z inside the box, and no box row is ever active.
# tests/test_poly_host.py asserts every one of these conditions.
SCALE_A = {(3, 2): 1.0, (6, 10): 1.25, (8, 11): 1.25, (12, 20): 0.6, (10, 27): 0.5, (20, 28): 0.5,
           (24, 27): 0.5, (24, 40): 0.5}


def family_a(n, m, fp32=False):
    """Random SPD H, random G (rows of unit expected norm) and F (nx = 3), x0
    and f1 per instance, rows
    -h1 <= G z <= h2 with h ~ U(0.2, 1), every fifth row without a lower side
    and every fifth (offset 2) without an upper one; box -0.7 <= z, z <= 0.5
    on the even entries only."""
    def make():
        rng = np.random.default_rng(1000 * n + m)
        M = rng.normal(size=(n, n))
        H = M @ M.T / n + 0.5 * np.eye(n)
        G = rng.normal(size=(m, n)) / np.sqrt(n)
        F = rng.normal(size=(n, NX_A))
        x0 = rng.normal(size=(BATCH_A, NX_A)) * SCALE_A[n, m]
        f1 = rng.normal(size=(BATCH_A, n)) * SCALE_A[n, m]
        hl = -rng.uniform(0.2, 1.0, size=(BATCH_A, m))
        hu = rng.uniform(0.2, 1.0, size=(BATCH_A, m))
        hl[:, 0::5] = -INF
        hu[:, 2::5] = INF
        ubz = np.where(np.arange(n) % 2 == 0, 0.5, INF)
        return Case(H, G, F, np.full(n, -0.7), ubz, x0, f1, hl, hu, fp32)
    return cached(("polyA", n, m, fp32), make)


# max_iter = 1: the (12, 20) instances (two or more active rows each, so none
# of them can end OPTIMAL after one iteration) followed by the same x0 and f1
# times 0.3 and times 0.05 (the last with an empty active set: OPTIMAL after
# no iteration at all)
MAXITER_SHAPE, MAXITER_FACTORS = (12, 20), (1.0, 0.3, 0.05)


def maxiter_case():
    def make():
        a = family_a(*MAXITER_SHAPE)
        k = len(MAXITER_FACTORS)
        return Case(a.H, a.G, a.F, a.lbz, a.ubz, np.vstack([t * a.x0 for t in MAXITER_FACTORS]),
                    np.vstack([t * a.f1 for t in MAXITER_FACTORS]), np.tile(a.hl, (k, 1)),
                    np.tile(a.hu, (k, 1)))
    return cached("polyMaxiter", make)


# ------------------------------------------------------------------ family B
def _spd(rng, n):
    M = rng.normal(size=(n, n))
    return M @ M.T / n + 0.5 * np.eye(n)


def _box_only(fp32):
    rng = np.random.default_rng(901)
    n, b = 9, 6
    F = rng.normal(size=(n, 2))
    ubz = np.where(np.arange(n) % 3 == 0, INF, 0.4)
    return Case(_spd(rng, n), None, F, np.full(n, -0.6), ubz, rng.normal(size=(b, 2)) * 2,
                rng.normal(size=(b, n)) * 2, None, None, fp32)


def _scalar(box, fp32):
    """n = m = 1: the row 1.5 z in [hl, hu] (and the box [-0.3, 0.4], parallel
    to it): instances free, at the row's lower / upper side, at the box, and
    one (the last) whose row is the most violated and is added first, after
    which the box row, dependent on it, takes its place."""
    f1 = np.array([[0.1], [3.0], [-3.0], [2.0], [-2.0], [0.0], [-3.0]])
    hl = np.array([[-1.0], [-0.3], [-1.0], [-0.9], [-INF], [0.15], [-1.0]])
    hu = np.array([[1.0], [1.0], [0.45], [INF], [0.9], [0.9], [0.75]])
    lbz, ubz = (np.array([-0.3]), np.array([0.4])) if box else (None, None)
    return Case(np.array([[2.0]]), np.array([[1.5]]), None, lbz, ubz, None, f1, hl, hu, fp32)


def _lower_only(fp32):
    rng = np.random.default_rng(903)
    n, m, b = 5, 4, 6
    return Case(_spd(rng, n), rng.normal(size=(m, n)), None, None, None, None,
                rng.normal(size=(b, n)) * 3, -rng.uniform(0.2, 1.0, size=(b, m)), None, fp32)


def _project_zero(fp32):
    """f = 0 and hl > 0: the projection of 0 onto the polytope in the H norm."""
    rng = np.random.default_rng(904)
    n, m, b = 5, 3, 6
    hl = rng.uniform(0.2, 1.0, size=(b, m))
    return Case(_spd(rng, n), rng.normal(size=(m, n)), None, None, None, None, np.zeros((b, n)),
                hl, hl + 1.0, fp32)


EQ_ROWS = (1, 3)


def _equality(fp32):
    rng = np.random.default_rng(905)
    n, m, b = 8, 5, 4
    hl = -rng.uniform(0.2, 1.0, size=(b, m))
    hu = rng.uniform(0.2, 1.0, size=(b, m))
    hl[:, EQ_ROWS] = hu[:, EQ_ROWS]
    return Case(_spd(rng, n), rng.normal(size=(m, n)), None, None, None, None,
                rng.normal(size=(b, n)) * 2, hl, hu, fp32)


def _dependent(fp32):
    """Duplicated rows, unit rows that duplicate box rows and scaled copies
    (tests/test_gpu_qp.py test_qp_dependent_rows), f large enough that the set
    saturates: the multipliers are not unique, z is."""
    rng = np.random.default_rng(5)
    n, b = 12, 8
    Qm, _ = np.linalg.qr(rng.normal(size=(n, n)))
    H = (Qm * np.geomspace(1.0, 50.0, n)) @ Qm.T
    G0 = rng.normal(size=(4, n))
    G = np.vstack([G0, G0, np.eye(n)[:3], 2 * G0[:2]])
    hu = np.concatenate([np.full(4, 0.3), np.full(4, 0.3), np.full(3, 0.2), np.full(2, 0.6)])
    return Case(H, G, None, np.full(n, -1.0), np.full(n, 1.0), None, rng.normal(size=(b, n)) * 30,
                -hu, hu, fp32)


# name -> (builder, y unique (compare it with the oracle's), run in fp32 too)
CASES_B = {
    "box_only": (_box_only, True, True),
    "scalar": (lambda fp32: _scalar(False, fp32), True, True),
    "scalar_box": (lambda fp32: _scalar(True, fp32), True, True),
    "lower_only": (_lower_only, True, True),
    "project_zero": (_project_zero, True, True),
    "equality": (_equality, True, True),
    "dependent": (_dependent, False, False),
}


def family_b(name, fp32=False):
    return cached(("polyB", name, fp32), lambda: CASES_B[name][0](fp32))
