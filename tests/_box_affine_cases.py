"""The oracle-side reference of the affine box loop (mpcqp_mpc_box_loop_affine)
and its scenarios, shared by tests/test_box_affine_host.py (reference only) and
tests/test_gpu_box_affine.py.

Per step the reference is oracle.qp.box_qp on

    min 1/2 z'Hz + (F x + g_t)'z,  lb <= z <= ub

with H, F from oracle.condense of the instance's plant, certified by
oracle.qp.kkt_box below 1e-9 * max(1, |f|), and the plant step x+ = A x + B
z[:nu] + w_t.  The helper rules (fp32 tolerance, bounds of an instance, the
per-step check at the device's own states, the random per-instance plants and
the FHC plant) are those of tests/test_gpu_loop_box.py, copied here.
"""
import numpy as np

from oracle import condense as oc
from oracle import qp as oq

EPS32 = float(np.finfo(np.float32).eps)

# (nx, nu, N): all three <NX, NU> instantiations of box_loop_kernel, block sizes
# 1, 2 (four waves per SIMD), 6 and 8, padded states and inputs; (4, 2, 10) is
# n = 20, block size 5: the one fp64 instantiation whose warm-started solve
# runs on the compare-and-select reductions (LoopKeyed, loop_box.hip)
SHAPES = [(1, 1, 3), (2, 1, 8), (2, 2, 11), (4, 1, 32), (3, 2, 16), (4, 2, 2), (4, 2, 10)]
FP32_SHAPES = [(2, 1, 8), (3, 2, 16), (4, 1, 32)]
B, T = 5, 6          # a second wave with one live group
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tol32(H):
    """Relative fp32 tolerance on z: max(2e-4, 3 * eps32 * cond(H)) with
    cond(H) <= 1e4."""
    cond = np.linalg.cond(H)
    assert cond <= 1e4, cond
    return max(2e-4, 3 * EPS32 * cond)


def bnd(v, i, n):
    """Bounds of instance i as an (n,) vector, or None."""
    if v is None:
        return None
    v = np.asarray(v, float)
    return np.broadcast_to(v[i] if v.ndim == 2 else v, (n,))


def row(v, t, i):
    """Step t, instance i of a (T, n) shared or (T, b, n) per-instance term; 0
    for None."""
    if v is None:
        return 0.0
    return v[t] if v.ndim == 2 else v[t, i]


def step(H, F, lb, ub, x, g=0.0):
    """(z, f): the oracle's argmin with f = F x + g, KKT-certified."""
    f = F @ x + g
    z = oq.box_qp(H, f, lb, ub)[0]
    kkt = oq.kkt_box(H, f, lb, ub, z)
    assert kkt < 1e-9 * max(1.0, np.abs(f).max()), kkt
    return z, f


def host_loop(A, Bm, H, F, lb, ub, x0, steps, g=None, w=None):
    """The oracle's own closed loop of one instance with g (steps, n) and w
    (steps, nx) (or None): xs (steps+1, nx), zs (steps, n)."""
    nu = Bm.shape[1]
    xs, zs = [np.asarray(x0, float)], []
    for t in range(steps):
        z, _ = step(H, F, lb, ub, xs[-1], 0.0 if g is None else g[t])
        zs.append(z)
        xs.append(A @ xs[-1] + Bm @ z[:nu] + (0.0 if w is None else w[t]))
    return np.array(xs), np.array(zs)


def check_episode(A, Bm, H, F, lb, ub, xs, us, zs, i, g=None, w=None, fp32=False):
    """Instance i of a device episode (xs (T+1, b, nx), us (T, b, nu), zs
    (T, b, n) as float64 arrays) against the oracle at the device's own
    states.  For every step t:
      zs[t] = argmin 1/2 z'Hz + (F xs[t] + g_t)'z over the box, to 1e-9 *
        max(1, |z_ref|) in fp64 and tol32(H) * max(1, |z_ref|) in fp32;
      us[t] is zs[t][:nu], bitwise;
      xs[t+1] = A xs[t] + B us[t] + w_t, to 1e-12 * (1 + |x|) in fp64 and to
        8 * eps32 * (|A||x| + |B||u| + |w|) in fp32.
    g, w: (T, n) / (T, b, n) and (T, b, nx), or None.  Returns the largest
    relative z error."""
    steps, nu, n = us.shape[0], us.shape[2], zs.shape[2]
    lbi, ubi = bnd(lb, i, n), bnd(ub, i, n)
    tol = tol32(H) if fp32 else 1e-9
    worst = 0.0
    for t in range(steps):
        x, u = xs[t, i], us[t, i]
        zr, _ = step(H, F, lbi, ubi, x, row(g, t, i))
        err = np.abs(zs[t, i] - zr).max() / max(1.0, np.abs(zr).max())
        worst = max(worst, err)
        assert err < tol, (i, t, err)
        assert np.array_equal(u, zs[t, i, :nu]), (i, t)
        wt = row(w, t, i)
        xn = A @ x + Bm @ u + wt
        if fp32:
            bound = 8 * EPS32 * (np.abs(A) @ np.abs(x) + np.abs(Bm) @ np.abs(u) + np.abs(wt))
            assert (np.abs(xs[t + 1, i] - xn) <= bound).all(), (i, t, xs[t + 1, i] - xn, bound)
        else:
            assert np.abs(xs[t + 1, i] - xn).max() < 1e-12 * (1 + np.abs(xn).max()), (i, t)
    return worst


# ---------------------------------------------- random per-instance plants
# seed offsets at which the scenario meets what tests/test_box_affine_host.py
# asks of it (cond(H) <= 1e4, active and free entries, g that matters)
SEED = 28


def problem(nx, nu, N):
    """Per-instance plants of spectral radius 1.02 and per-instance bounds that
    differ along the horizon (x 4 on odd stages), with infinite and fixed
    entries; g (T, B, n) random with the scale of F x0, w (T, B, nx) random and
    small; the oracle's own closed loops with g and w ("ref": xs, zs per
    instance) and with g = 0 from the same states ("z0")."""
    def make():
        rng = np.random.default_rng(SEED + 10000 * nx + 1000 * nu + N)
        b, n = B, N * nu
        A = rng.normal(size=(b, nx, nx)) * (0.8 / np.sqrt(nx)) + 0.4 * np.eye(nx)
        A *= (1.02 / np.abs(np.linalg.eigvals(A)).max(axis=-1))[:, None, None]
        Bm = rng.normal(size=(b, nx, nu))
        M = rng.normal(size=(nx, nx))
        Q = M @ M.T / nx + 0.2 * np.eye(nx)
        R = np.diag(rng.uniform(0.1, 1.0, nu))
        x0 = 3 * rng.normal(size=(b, nx))
        ub = rng.uniform(0.05, 0.3, (b, N, nu))
        lb = -rng.uniform(0.05, 0.3, (b, N, nu))
        ub[:, 1::2] *= 4
        lb[:, 1::2] *= 4
        lb, ub = lb.reshape(b, n), ub.reshape(b, n)
        lb[rng.random((b, n)) < 0.10] = -np.inf
        ub[rng.random((b, n)) < 0.10] = np.inf
        fx = rng.random((b, n)) < 0.05
        lb[fx] = ub[fx] = 0.02
        p = dict(A=A, B=Bm, Q=Q, R=R, Qf=3 * Q, N=N, x0=x0, lb=lb, ub=ub)
        p["cd"] = [oc.condense(A[i], Bm[i], Q, R, 3 * Q, N) for i in range(b)]
        assert max(np.linalg.cond(d["H"]) for d in p["cd"]) <= 1e4
        rg = np.random.default_rng(4242 + 100 * nx + 10 * nu + N)
        scale = max(np.abs(p["cd"][i]["F"] @ x0[i]).max() for i in range(b))
        p["g"] = 0.5 * scale * rg.normal(size=(T, b, n))
        p["w"] = 0.05 * rg.normal(size=(T, b, nx))
        p["ref"], p["z0"] = [], []
        for i in range(b):
            d = p["cd"][i]
            xs, zs = host_loop(A[i], Bm[i], d["H"], d["F"], lb[i], ub[i], x0[i], T, p["g"][:, i],
                               p["w"][:, i])
            p["ref"].append((xs, zs))
            p["z0"].append(np.array([step(d["H"], d["F"], lb[i], ub[i], xs[t])[0]
                                     for t in range(T)]))
        return p
    return cached(("problem", nx, nu, N), make)


# ------------------------------------------- setpoint tracking on the FHC plant
def fhc_plant():
    ts = 0.5                                        # FHC.py:44-48, config 2
    A = np.array([[1.0, ts], [0.0, 1.0]])
    Bm = np.array([[0.0], [-ts]])
    C = np.array([[1.0], [-2.0 / 3.0]])
    Q = C @ C.T + 1e-3 * np.eye(2)
    return A, Bm, Q, np.array([[0.1]]), Q.copy()


SP_N, SP_T = 20, 30
SP_PSTAR = 8.0                  # the setpoint (p*, 0): far enough for |u| = 1 at first
# |x_T - x_ref| (max norm) that the oracle's own loop reaches at the last step,
# pinned from tests/test_box_affine_host.py::test_setpoint_converges, and the
# bound of the device's lti_box_mpc_loop there: a factor 10 over it
SP_ORACLE_LAST = 3.0e-7        # 2.99e-7
SP_LAST_BOUND = 10 * SP_ORACLE_LAST


def tracking_g(Gam, Q, R, Qf, N, steps, x_ref=None, u_ref=None):
    """g (steps, n) by the definition: g_t = -Gam' Qhat rbar_t - Rhat ubar_t,
    rbar_t = x_ref[t+1 : t+N+1] (x_ref (steps+N+1, nx)), ubar_t = u_ref[t : t+N]
    (u_ref (steps+N, nu)), Qhat = blkdiag(Q, .., Q, Qf), Rhat = blkdiag(R, .., R)."""
    nx, nu = Q.shape[0], R.shape[0]
    Qhat = np.zeros((N * nx, N * nx))
    Rhat = np.zeros((N * nu, N * nu))
    for k in range(N):
        Qhat[k * nx:(k + 1) * nx, k * nx:(k + 1) * nx] = Qf if k == N - 1 else Q
        Rhat[k * nu:(k + 1) * nu, k * nu:(k + 1) * nu] = R
    g = np.zeros((steps, N * nu))
    for t in range(steps):
        if x_ref is not None:
            g[t] -= Gam.T @ Qhat @ x_ref[t + 1:t + N + 1].reshape(-1)
        if u_ref is not None:
            g[t] -= Rhat @ u_ref[t:t + N].reshape(-1)
    return g


def setpoint():
    """The FHC double integrator, |u| <= 1, N = 20, tracking x_ref = (p*, 0)
    with u_ref = 0 from x0 = 0: dict(A, B, Q, R, Qf, cd, x_ref (T+N+1, 2), g
    (T, n), xs, zs of the oracle's own loop)."""
    def make():
        A, Bm, Q, R, Qf = fhc_plant()
        cd = oc.condense(A, Bm, Q, R, Qf, SP_N)
        x_ref = np.tile([SP_PSTAR, 0.0], (SP_T + SP_N + 1, 1))
        g = tracking_g(cd["Gam"], Q, R, Qf, SP_N, SP_T, x_ref, np.zeros((SP_T + SP_N, 1)))
        xs, zs = host_loop(A, Bm, cd["H"], cd["F"], -np.ones(SP_N), np.ones(SP_N), np.zeros(2),
                           SP_T, g)
        return dict(A=A, B=Bm, Q=Q, R=R, Qf=Qf, cd=cd, x_ref=x_ref, g=g, xs=xs, zs=zs)
    return cached("setpoint", make)
