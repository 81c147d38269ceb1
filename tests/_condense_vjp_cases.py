"""Shared by tests/test_condense_vjp_host.py and tests/test_gpu_condense_vjp.py:
the NumPy closed form of the adjoint of condensing (mpcqp_condense_vjp,
include/mpcqp_diff.h) and the scenarios it is checked on.

With n = N nu, the stacked rows S = [Gam, Phi, xbar] (N nx x (n + nx + 1)) of
oracle.condense, S_{-1} = [0, I, x0], GY = [Ghat, gF, gf] (Ghat symmetric, Ghat_ii
= gH_ii, Ghat_ij = gH_ij / 2 from the packed gH) and Q_k = Q (k < N-1), Qf (k =
N-1):

    for k = N-1 .. 0:
        T_k   = Gam_k GY S_k'                   gQf = T_{N-1}, gQ = sum_{k<N-1} T_k
        GS_k  = Q_k' Gam_k GY;  GS_k[:, :n] += Q_k S_k GY'
        Lam_k = GS_k + A_{k+1}' Lam_{k+1}       (Lam_N = 0)
        gA_k = Lam_k S_{k-1}',  gB_k = Lam_k[:, k nu : (k+1) nu],  gc_k = Lam_k[:, -1]
    gx0 = (A_0' Lam_0)[:, -1],  gR = sum_k Ghat[k nu.., k nu..]

gA and gB are summed over k for a time-invariant plant; gQ, gQf and gR are
symmetrised.
"""
import numpy as np

from oracle import condense as oc

# (nx, nu, N) of the kernel tests: the smallest problem, one stage with the
# widest state and input, the 2loop shape (2, 1, 20), odd sizes, and both ways
# to the limit n = 32
SHAPES = [(1, 1, 1), (4, 2, 1), (2, 1, 3), (2, 1, 20), (3, 2, 4), (4, 2, 16), (4, 1, 32)]
HOST_SHAPES = [(1, 1, 1, False), (2, 1, 3, False), (3, 2, 4, True), (4, 2, 16, True)]
BATCH = 7
OUTPUTS = ("gA", "gB", "gQ", "gR", "gQf", "gc", "gx0")


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def ghat(gH, n):
    """The symmetric matrix of a gradient on the packed lower entries."""
    G = np.zeros((n, n))
    G[np.tril_indices(n)] = gH
    return 0.5 * (G + G.T)


def closed_form(A, Bm, Q, R, Qf, N, x0=None, c=None, gH=None, gF=None, gf=None):
    """One instance.  A (nx, nx) or (N, nx, nx), Bm likewise; gH packed, gF
    (n, nx), gf (n,), each None = 0.  dict of OUTPUTS in the shapes of the inputs
    (gc (N, nx), valid also for c = None)."""
    A, Bm = np.asarray(A, float), np.asarray(Bm, float)
    tv = A.ndim == 3
    nx, nu = Bm.shape[-2:]
    n = N * nu
    C = n + nx + 1
    cd = oc.condense(A, Bm, Q, R, Qf, N, x0=x0, c=c)
    S = np.concatenate([cd["Gam"], cd["Phi"], cd["xbar"][:, None]], axis=1)
    x0v = np.zeros(nx) if x0 is None else np.asarray(x0, float)
    Sm1 = np.concatenate([np.zeros((nx, n)), np.eye(nx), x0v[:, None]], axis=1)
    GY = np.zeros((n, C))
    if gH is not None:
        GY[:, :n] = ghat(gH, n)
    if gF is not None:
        GY[:, n:n + nx] = gF
    if gf is not None:
        GY[:, -1] = gf
    Ak = lambda k: A[k] if tv else A  # noqa: E731
    blk = lambda k: S[k * nx:(k + 1) * nx]  # noqa: E731
    gA = np.zeros((N, nx, nx))
    gB = np.zeros((N, nx, nu))
    gc = np.zeros((N, nx))
    gQ = np.zeros((nx, nx))
    gQf = np.zeros((nx, nx))
    lam = np.zeros((nx, C))
    for k in range(N - 1, -1, -1):
        Sk = blk(k)
        Qk = np.asarray(Qf if k == N - 1 else Q, float)
        P = Sk[:, :n] @ GY
        Tk = P @ Sk.T
        if k == N - 1:
            gQf = Tk
        else:
            gQ = gQ + Tk
        GS = Qk.T @ P
        GS[:, :n] += Qk @ Sk @ GY.T
        lam = GS + (Ak(k + 1).T @ lam if k < N - 1 else 0.0)
        gA[k] = lam @ (blk(k - 1) if k > 0 else Sm1).T
        gB[k] = lam[:, k * nu:(k + 1) * nu]
        gc[k] = lam[:, -1]
    gx0 = (Ak(0).T @ lam)[:, -1]
    Gh = GY[:, :n]
    gR = sum(Gh[k * nu:(k + 1) * nu, k * nu:(k + 1) * nu] for k in range(N))
    return dict(gA=gA if tv else gA.sum(0), gB=gB if tv else gB.sum(0), gQ=sym(gQ), gR=sym(gR),
                gQf=sym(gQf), gc=gc, gx0=gx0)


def scenario(nx, nu, N, tv, dtype=np.float64, batch=BATCH, seed=0):
    """``batch`` instances: plants scaled to spectral radius <= 1 (every stage
    matrix of a time-varying one), Q, Qf and R SPD, x0, c and the upstream
    gradients standard normal, all rounded to ``dtype`` and returned as float64
    arrays: dict(A, B, Q, R, Qf, x0, c, gH, gF, gf) with a leading batch
    dimension."""
    rng = np.random.default_rng(9000 + 1000 * nx + 100 * nu + N + (50 if tv else 0) + seed)
    n = N * nu
    st = (batch, N) if tv else (batch,)
    A = rng.standard_normal(st + (nx, nx))
    A *= (rng.uniform(0.6, 1.0, st) / np.abs(np.linalg.eigvals(A)).max(axis=-1))[..., None, None]
    Bm = rng.standard_normal(st + (nx, nu))

    def spd(k):
        M = rng.standard_normal((batch, k, k))
        return M @ np.swapaxes(M, -1, -2) / k + 0.5 * np.eye(k)

    p = dict(A=A, B=Bm, Q=spd(nx), R=spd(nu), Qf=spd(nx), x0=rng.standard_normal((batch, nx)),
             c=rng.standard_normal((batch, N, nx)),
             gH=rng.standard_normal((batch, n * (n + 1) // 2)),
             gF=rng.standard_normal((batch, n, nx)), gf=rng.standard_normal((batch, n)))
    p = {k: v.astype(dtype).astype(np.float64) for k, v in p.items()}
    for k in ("Q", "R", "Qf"):   # rounding keeps symmetry; say so
        assert np.array_equal(p[k], np.swapaxes(p[k], -1, -2))
    return p


def reference(p, N, i, *, c=True, x0=True, ups=("gH", "gF", "gf"), shared=False):
    """closed_form of instance i of a scenario (of instance 0's plant, weights,
    c and x0 when ``shared``), with the upstream gradients named in ``ups``."""
    j = 0 if shared else i
    return closed_form(p["A"][j], p["B"][j], p["Q"][j], p["R"][j], p["Qf"][j], N,
                       x0=p["x0"][j] if x0 else None, c=p["c"][j] if c else None,
                       **{k: p[k][i] for k in ups})


def rel_err(dev, ref):
    """max|dev - ref| / (1 + max|ref|)."""
    return float(np.abs(np.asarray(dev, float) - ref).max() / (1.0 + np.abs(ref).max()))
