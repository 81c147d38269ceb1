"""The oracle-side reference of the soft poly loop (mpcqp_mpc_poly_loop_soft)
and its scenarios, shared by tests/test_poly_soft_host.py (reference only) and
tests/test_gpu_poly_soft.py.

Per step the reference is oracle.qp.poly_qp on the QP with explicit slacks

    min 1/2 z'Hz + (F x)'z + sum_i ( rho_i eps_i + 1/2 sigma_i eps_i^2 )
    s.t.  C_i z - eps_i <= hi_i,  -C_i z - eps_i <= -lo_i,  -eps_i <= 0   (soft rows)
          lo <= C z <= hi                                                  (hard rows, box)

in the variables [z; eps over the soft rows], Hessian blkdiag(H, diag(sigma)),
gradient [F x; rho], certified by oracle.qp.kkt_poly below KKT_TOL * scale.
Bounds, plants and scenarios come from tests/_poly_loop_cases.LoopQP.
"""
import numpy as np

import _poly_loop_cases as pc
from model_predictive_control_amd.problems import Problem, Problem3
from oracle import qp as oq

KKT_TOL = 1e-9
SOFTENED = 1 << 26

# test 1: (rho, sigma) on every state row, the input box hard
PENALTIES = [(50.0, 1.0), (0.0, 100.0), (1000.0, 0.01), (5.0, 10.0)]


class SoftQP:
    """A LoopQP whose rows i < m with finite rho[i] are soft.  Has what
    _poly_loop_cases.check_episode reads (step()[0], A, B, nu)."""

    def __init__(self, qp, rho, sigma):
        self.qp = qp
        self.rho = np.broadcast_to(np.asarray(rho, float), (qp.m,)).copy()
        self.sigma = np.broadcast_to(np.asarray(sigma, float), (qp.m,)).copy()
        self.soft = np.nonzero(np.isfinite(self.rho))[0]
        self.A, self.B, self.nu, self.n, self.m, self.mt = qp.A, qp.B, qp.nu, qp.n, qp.m, qp.mt

    def step(self, x, hl=None, hu=None):
        """(z, y, eps, kkt/scale): the certified solution at state x; y (mt,)
        the signed row multipliers (> 0 at the upper bound), eps (m,) the
        slacks (0 on hard rows).  Raises ValueError when the QP is empty."""
        q = self.qp
        lo, hi = q.bounds(x, hl, hu)
        n, ns = q.n, self.soft.size
        col = {int(r): n + j for j, r in enumerate(self.soft)}
        rows, rhs, owner = [], [], []
        for sgn, bnd in ((1.0, hi), (-1.0, -lo)):
            for r in np.nonzero(np.isfinite(bnd))[0]:
                a = np.zeros(n + ns)
                a[:n] = sgn * q.Call[r]
                if int(r) in col:
                    a[col[int(r)]] = -1.0
                rows.append(a)
                rhs.append(bnd[r])
                owner.append((int(r), sgn))
        for j in range(ns):
            a = np.zeros(n + ns)
            a[n + j] = -1.0
            rows.append(a)
            rhs.append(0.0)
        C, d = np.array(rows), np.array(rhs)
        Ha = np.zeros((n + ns, n + ns))
        Ha[:n, :n] = q.H
        Ha[n:, n:] = np.diag(self.sigma[self.soft])
        f = np.concatenate([q.F @ x, self.rho[self.soft]])
        v, lam, _ = oq.poly_qp(Ha, f, C, d)
        scale = max(1.0, np.abs(d).max(initial=0.0), np.abs(f).max(initial=0.0))
        kkt = oq.kkt_poly(Ha, f, C, d, v, lam)
        assert kkt < KKT_TOL * scale, (kkt, scale)
        y = np.zeros(q.mt)
        for (r, sgn), lm in zip(owner, lam):
            y[r] += sgn * lm
        eps = np.zeros(q.m)
        eps[self.soft] = v[n:]
        return v[:n], y, eps, kkt / scale

    def host_loop(self, x0, T, w=None):
        """The reference's own closed loop: xs, zs, ys, eps."""
        q = self.qp
        xs = np.zeros((T + 1, q.nx))
        zs, ys, es = np.zeros((T, q.n)), np.zeros((T, q.mt)), np.zeros((T, q.m))
        xs[0] = x0
        for t in range(T):
            zs[t], ys[t], es[t], _ = self.step(xs[t])
            xs[t + 1] = q.A @ xs[t] + q.B @ zs[t, :q.nu] + (0.0 if w is None else w[t])
        return xs, zs, ys, es


def regimes(sq, y):
    """(soft-active, hard-active) masks of the m rows for multipliers y,
    decided well away from the switch: |y| > rho (1 + 1e-6) + 1e-9 is
    soft-active, 1e-9 < |y| < rho (1 - 1e-6) hard-active (soft rows only)."""
    a = np.abs(y[..., :sq.m])
    fin = np.isfinite(sq.rho)
    rho = np.where(fin, sq.rho, 0.0)
    return fin & (a > rho * (1 + 1e-6) + 1e-9), fin & (a > 1e-9) & (a < rho * (1 - 1e-6))


def check_slacks(sq, x, z, y, eps, word, hl=None, hu=None, tol=1e-8):
    """One step of a device episode against its own plan z: the slack is the
    row's violation, the status bit says whether there is one, y is stationary
    and each row is in the state its multiplier says."""
    q = sq.qp
    lo, hi = q.bounds(x, hl, hu)
    cz = q.Call @ z
    m = q.m
    viol = np.maximum(0.0, np.maximum(cz[:m] - hi[:m], lo[:m] - cz[:m]))
    fb = lambda b: np.where(np.isfinite(b), np.abs(b), 0.0)  # noqa: E731
    bound = tol * (1 + np.maximum(fb(lo[:m]), fb(hi[:m])) + np.abs(cz[:m]))
    assert (np.abs(eps - viol) <= bound).all(), (eps, viol)
    assert bool(word & SOFTENED) == bool((eps > 0).any())
    f = q.F @ x
    scale = max(1.0, np.abs(f).max(), np.abs(y).max())
    assert np.abs(q.H @ z + f + q.Call.T @ y).max() < tol * scale
    rho = np.concatenate([sq.rho, np.full(q.mt - m, np.inf)])
    sig = np.concatenate([sq.sigma, np.ones(q.mt - m)])
    ab = tol * (1 + np.maximum(fb(lo), fb(hi)) + np.abs(cz))
    for i in range(q.mt):
        ay = abs(y[i])
        b = hi[i] if y[i] > 0 else lo[i]
        out = (cz[i] - b) if y[i] > 0 else (b - cz[i])      # violation past the active bound
        if ay == 0:
            assert lo[i] - ab[i] <= cz[i] <= hi[i] + ab[i], i
        elif ay <= rho[i]:
            assert abs(out) <= ab[i], (i, out)
        else:
            assert abs(out - (ay - rho[i]) / sig[i]) <= ab[i] * max(1.0, 1.0 / sig[i]), (i, out)


# ---------------------------------------------------------------- scenarios
def feasibility_batch(N):
    """Test 1: the INFEASIBLE_CASES of horizon N plus the feasible neighbour."""
    X0 = np.array([x0 for n_, x0, _ in pc.INFEASIBLE_CASES if n_ == N] + [pc.FEASIBLE_NEIGHBOUR])
    return pc.infeasible_qp(N), X0


def feasibility_reference(N, rho, sigma):
    def make():
        qp, X0 = feasibility_batch(N)
        sq = SoftQP(qp, rho, sigma)
        return sq, X0, [sq.host_loop(x0, pc.T_EPISODE) for x0 in X0]
    return pc.cached(("soft-feas", N, rho, sigma), make)


SHAPE_SCALE, SHAPE_RHO, SHAPE_SIGMA = 0.3, 0.02, 10.0


def shape_soft(nx, nu, N, rho=SHAPE_RHO):
    """Test 5: shape_problem with its state bounds scaled by 0.3."""
    def make():
        p = pc.shape_problem(nx, nu, N)
        q = p["qp"]
        q2 = pc.LoopQP(q.H, q.F, q.G, q.E, SHAPE_SCALE * q.hl, SHAPE_SCALE * q.hu, q.lbz, q.ubz,
                       q.A, q.B)
        sq = SoftQP(q2, rho, SHAPE_SIGMA)
        return sq, p["x0"], [sq.host_loop(x0, pc.SHAPE_T) for x0 in p["x0"]]
    return pc.cached(("soft-shape", nx, nu, N, rho), make)


DRIFT_RHO, DRIFT_SIGMA = 300.0, 1.0
DRIFT_STEPS = sorted(set(range(0, pc.T_DRIFT, 10)) | {63, 64, 65, 127, 128, 129, 191, 192, 193})


def drift_soft():
    """Test 6: the drift scenario with 1.5 x the disturbance."""
    def make():
        qp = pc.session_qp(Problem(), 5)
        w = pc.drift_w() * 1.5
        sq = SoftQP(qp, DRIFT_RHO, DRIFT_SIGMA)
        return sq, w, [sq.host_loop(np.zeros(2), pc.T_DRIFT, w=w[:, i]) for i in range(2)]
    return pc.cached("soft-drift", make)


C4_RHO, C4_SIGMA = 0.05, 10.0


def config4_soft():
    def make():
        p = pc.config4_problem()
        sq = SoftQP(p["qp"], C4_RHO, C4_SIGMA)
        return sq, p["x0"], [sq.host_loop(x0, pc.SHAPE_T) for x0 in p["x0"]]
    return pc.cached("soft-config4", make)


def mixed_soft(N=5):
    """Test 4: position rows soft (50, 1), velocity rows hard, per-row vectors."""
    qp, X0 = feasibility_batch(N)
    rho = np.tile([50.0, np.inf], N)
    sigma = np.tile([1.0, 1.0], N)
    return SoftQP(qp, rho, sigma), X0


def session_problem(name):
    return {"Problem": Problem, "Problem3": Problem3}[name]()
