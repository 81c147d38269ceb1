"""The oracle-side reference of the affine poly loop
(mpcqp_mpc_poly_loop_affine) and its scenarios, shared by
tests/test_poly_affine_host.py (reference only) and
tests/test_gpu_poly_affine.py.

Per step the reference is oracle.qp.poly_qp on

    min 1/2 z'Hz + (F x + g)'z   s.t.  hl - E x - e <= G z <= hu - E x - e,
                                       lbz <= z <= ubz

certified by oracle.qp.kkt_poly below 1e-9 * scale, exactly as
tests/_poly_loop_cases.LoopQP.step (g = e = 0 is that problem).
"""
import numpy as np

import _poly_loop_cases as pc
import _poly_soft_cases as sc
from model_predictive_control_amd.problems import Problem
from oracle import condense as oc
from oracle import qp as oq


class AffineQP(pc.LoopQP):
    """A LoopQP whose step takes a linear term g in the gradient and a shift e
    of the first m rows' bounds."""

    @classmethod
    def of(cls, q):
        return cls(q.H, q.F, q.G if q.m else None, q.E, q.hl, q.hu, q.lbz if q.nbox else None,
                   q.ubz if q.nbox else None, q.A, q.B)

    def affine_bounds(self, x, e=None, hl=None, hu=None):
        lo, hi = self.bounds(x, hl, hu)
        if e is not None:
            lo[:self.m] = lo[:self.m] - e
            hi[:self.m] = hi[:self.m] - e
        return lo, hi

    def step(self, x, g=None, e=None, hl=None, hu=None):
        """(z, y, act) as LoopQP.step, with f = F x + g and the first m rows'
        bounds moved by -e.  Raises ValueError when the QP is empty."""
        lo, hi = self.affine_bounds(x, e, hl, hu)
        ku, kl = np.isfinite(hi), np.isfinite(lo)
        C = np.vstack([self.Call[ku], -self.Call[kl]])
        d = np.concatenate([hi[ku], -lo[kl]])
        f = self.F @ x + (0.0 if g is None else g)
        z, lam, _ = oq.poly_qp(self.H, f, C, d)
        scale = max(1.0, np.abs(d).max(initial=0.0), np.abs(f).max(initial=0.0))
        kkt = oq.kkt_poly(self.H, f, C, d, z, lam)
        assert kkt < 1e-9 * scale, (kkt, scale)
        y = np.zeros(self.mt)
        y[ku] += lam[:ku.sum()]
        y[kl] -= lam[ku.sum():]
        act = np.where(y > 0, 2, np.where(y < 0, 1, 0))
        return z, y, act

    def host_loop(self, x0, T, g=None, e=None):
        """The oracle's own closed loop with g (T, n), e (T, m): xs, zs, acts,
        fail = the first step whose QP is empty (None if none)."""
        xs = np.full((T + 1, self.nx), np.nan)
        zs = np.full((T, self.n), np.nan)
        acts = np.full((T, self.mt), -1)
        xs[0] = x0
        for t in range(T):
            try:
                zs[t], _, acts[t] = self.step(xs[t], None if g is None else g[t],
                                              None if e is None else e[t])
            except ValueError as err:
                assert "infeasible" in str(err)
                return xs, zs, acts, t
            xs[t + 1] = self.A @ xs[t] + self.B @ zs[t, :self.nu]
        return xs, zs, acts, None


class AffineSoftQP:
    """The soft reference (_poly_soft_cases.SoftQP) with g and e: the same QP
    with explicit slacks, posed in the augmented state [x; 1] with F_aug = [F,
    g] (so that F_aug [x; 1] = F x + g) and the row bounds moved by -e."""

    def __init__(self, q, rho, sigma):
        self.q, self.rho, self.sigma = q, rho, sigma
        self.A, self.B, self.nu = q.A, q.B, q.nu

    def step(self, x, g=None, e=None):
        """(z, y, eps, kkt/scale) as SoftQP.step."""
        q = self.q
        g = np.zeros(q.n) if g is None else g
        e = np.zeros(q.m) if e is None else e
        Eaug = None if q.E is None else np.hstack([q.E, np.zeros((q.m, 1))])
        qa = pc.LoopQP(q.H, np.hstack([q.F, g[:, None]]), q.G if q.m else None, Eaug, q.hl - e,
                       q.hu - e, q.lbz if q.nbox else None, q.ubz if q.nbox else None, q.A, q.B)
        return sc.SoftQP(qa, self.rho, self.sigma).step(np.append(x, 1.0))


def check_affine_episode(qp, xs, us, zs, i, g, e, ys=None, tol=1e-8, fp32=False, n_steps=None):
    """Instance i of a device episode against the oracle at the device's own
    states, by the rules of _poly_loop_cases.check_episode, with g (T, n) and e
    (T, m) of that instance (or None); with ys also the multipliers:
    stationarity H z + F x + g + C'y = 0 and the sign convention.  Returns the
    largest relative z error."""
    worst = 0.0
    for t in range(us.shape[0] if n_steps is None else n_steps):
        x, u = xs[t, i], us[t, i]
        gt = None if g is None else g[t]
        et = None if e is None else e[t]
        zr = qp.step(x, gt, et)[0]
        err = np.abs(zs[t, i] - zr).max() / max(1.0, np.abs(zr).max())
        worst = max(worst, err)
        assert err < tol, (i, t, err)
        assert np.array_equal(u, zs[t, i, :qp.nu]), (i, t)
        xn = qp.A @ x + qp.B @ u
        if fp32:
            bound = 8 * pc.EPS32 * (np.abs(qp.A) @ np.abs(x) + np.abs(qp.B) @ np.abs(u))
            assert (np.abs(xs[t + 1, i] - xn) <= bound).all(), (i, t)
        else:
            assert np.abs(xs[t + 1, i] - xn).max() < 1e-12 * (1 + np.abs(xn).max()), (i, t)
        if ys is not None:
            z, y = zs[t, i], ys[t, i]
            f = qp.F @ x + (0.0 if gt is None else gt)
            lo, hi = qp.affine_bounds(x, et)
            scale = max(1.0, np.abs(f).max(), np.abs(y).max())
            assert np.abs(qp.H @ z + f + qp.Call.T @ y).max() < tol * scale, (i, t)
            cz = qp.Call @ z
            up, dn = y > 0, y < 0
            assert (np.abs(cz[up] - hi[up]) < tol * (1 + np.abs(hi[up]))).all(), (i, t)
            assert (np.abs(cz[dn] - lo[dn]) < tol * (1 + np.abs(lo[dn]))).all(), (i, t)
    return worst


# ------------------------------------------------------------- S1: tracking
S1_N, S1_T = 5, 24
S1_X0 = np.array([(-40.0, 0.0), (-60.0, 25.0), (-5.0, 8.0)])
S1_ACTIVE = {"ramp": (18, 24, 21), "sine": (4, 8, 10)}   # steps with an active state row


def s1_reference_signal(kind, problem=None, T=S1_T, N=S1_N):
    """x_ref (T+N+1, 2): the position reference and its numerical derivative."""
    Ts = (problem or Problem()).Ts
    k = np.arange(T + N + 1)
    pos = np.minimum(-40.0 + 6.0 * k, 8.0) if kind == "ramp" else -20.0 + 25.0 * np.sin(0.35 * k)
    return np.stack([pos, np.gradient(pos) / Ts], axis=1)


def tracking_g(problem, N, T, x_ref, Qf=None):
    """g (T, n) for a state reference x_ref (T+N+1, nx), from the oracle's Gam
    by the definition: g_t = -Gam' Qhat rbar_t, rbar_t = x_ref[t+1 : t+N+1]."""
    Q = np.asarray(problem.Q, float)
    Qf = Q if Qf is None else Qf
    d = oc.condense(problem.A, problem.B, Q, np.asarray(problem.R, float), Qf, N)
    nx = problem.n_state
    Qhat = np.zeros((N * nx, N * nx))
    for k in range(N):
        Qhat[k * nx:(k + 1) * nx, k * nx:(k + 1) * nx] = Qf if k == N - 1 else Q
    return np.stack([-d["Gam"].T @ Qhat @ x_ref[t + 1:t + N + 1].reshape(-1) for t in range(T)])


def s1_reference(kind):
    """(qp, x_ref, g, [host_loop of every S1_X0 entry])."""
    def make():
        pr = Problem()
        qp = AffineQP.of(pc.session_qp(pr, S1_N))
        x_ref = s1_reference_signal(kind, pr)
        g = tracking_g(pr, S1_N, S1_T, x_ref)
        return qp, x_ref, g, [qp.host_loop(x0, S1_T, g) for x0 in S1_X0]
    return pc.cached(("affine-s1", kind), make)


# ----------------------------------------------------- S2: every block size
def s2_case(nx, nu, N):
    """shape_problem with random g (T, B, n) and e (T, B, m): (qp, x0, g, e,
    [host_loop per instance])."""
    def make():
        p = pc.shape_problem(nx, nu, N)
        qp = AffineQP.of(p["qp"])
        x0 = p["x0"]
        T, B = pc.SHAPE_T, pc.SHAPE_B
        rng = np.random.default_rng(4242 + 100 * nx + 10 * nu + N)
        g = 0.5 * np.abs(qp.F @ x0.T).max() * rng.normal(size=(T, B, qp.n))
        fin = np.isfinite(qp.hu)
        e = np.zeros((T, B, qp.m))
        e[:, :, fin] = 0.1 * qp.hu[fin] * rng.uniform(-1, 1, size=(T, B, int(fin.sum())))
        return qp, x0, g, e, [qp.host_loop(x0[i], T, g[:, i], e[:, i]) for i in range(B)]
    return pc.cached(("affine-s2", nx, nu, N), make)


# ------------------------------------- S3: loss of feasibility under tracking
S3_T = 16
S3_CASES = [((-60.0, 25.0), 4), ((-30.0, 10.0), 3), ((-100.0, 0.0), 14), ((-40.0, 0.0), 7)]
S3_SOFT = (50.0, 1.0)


def s3_reference():
    """(qp, g, [host_loop of every S3_CASES x0])."""
    def make():
        pr = Problem(u_min=-2.0)
        qp = AffineQP.of(pc.session_qp(pr, S1_N))
        g = tracking_g(pr, S1_N, S3_T, s1_reference_signal("ramp", pr, S3_T))
        return qp, g, [qp.host_loop(np.array(x0), S3_T, g) for x0, _ in S3_CASES]
    return pc.cached("affine-s3", make)
