"""The fused box kernel's one-loop setup: W~ by rows and f in Lyapunov form.

mpcqp_mpc_box (four QPs per wavefront) generates W~ = W diag(chol(S_k^{-1}))
row by row, backward in the column stage j, inside the Riccati loop:
    W~[(t,a), (j,:)] = Psi_j(t)[a] B_j L_j   (t > j),   L_j[a]  (t = j),   0  (t < j),
    Psi_{j-1}(t) = Psi_j(t) (A_j + B_j K_j),   Psi_{j-1}(j) = K_j,
and f from the x0-independent backward form of the adjoint,
    Pi_k = Q + A_k' Pi_{k+1} A_k,  pi_k = A_k'(Pi_{k+1} c_k + pi_{k+1}),  Pi_N = Qf, pi_N = 0,
    f_k = (B_k' Pi_{k+1}) xbar_{k+1} + B_k' pi_{k+1}.
Both are restated here in NumPy and checked on the host against the explicit
condensing; the kernel is checked against the oracle (explicit condensing +
active set) at the smallest shapes at which the loop takes another path, and
against the one-QP-per-wavefront kernel (MPCQP_KERNEL=wave).
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import condense as oc
from oracle import qp as oq
from oracle import session1 as s1


def _t(a, dev, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _plants(rng, nx, nu, N, tv, batch=None):
    """Random (marginally) stable plants and weights, Qf = 3 Q (as
    test_gpu_mpc_box_factor.py draws them); batch=None gives one instance."""
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


def _cfg2_plant():
    A, B, Q, R, Pf, _ = s1.fhc_setup()
    return A, B, Q, R.reshape(1, 1), Pf


def _rows_and_f(A, B, Q, R, Qf, N, x0, c):
    """(W~, f) by the row recursion and the Lyapunov-form adjoint, one
    backward loop plus the forward free response."""
    nx, nu = B.shape[-2:]
    n = N * nu
    st = lambda M, k: M[k] if M.ndim == 3 else M  # noqa: E731
    P, Pi, pi = Qf, Qf, np.zeros(nx)
    psi = np.zeros((n, nx))
    Wt = np.zeros((n, n))
    g, h = [None] * N, [None] * N
    for j in range(N - 1, -1, -1):
        Aj, Bj = st(A, j), st(B, j)
        Si = np.linalg.inv(R + Bj.T @ P @ Bj)
        L = np.linalg.cholesky(Si)
        K = -Si @ Bj.T @ P @ Aj
        Acl = Aj + Bj @ K
        for r in range(n):
            t, a = divmod(r, nu)
            if t == j:
                Wt[r, j * nu:(j + 1) * nu] = L[a]
                psi[r] = K[a]
            elif t > j:
                Wt[r, j * nu:(j + 1) * nu] = psi[r] @ Bj @ L
                psi[r] = psi[r] @ Acl
        g[j], h[j] = Bj.T @ Pi, Bj.T @ pi
        cj = np.zeros(nx) if c is None else c[j]
        pi = Aj.T @ (Pi @ cj + pi)
        Pi = Q + Aj.T @ Pi @ Aj
        P = Q + Aj.T @ P @ Aj + Aj.T @ P @ Bj @ K
    f = np.zeros(n)
    x = np.asarray(x0, float)
    for k in range(N):
        x = st(A, k) @ x + (0.0 if c is None else c[k])
        f[k * nu:(k + 1) * nu] = g[k] @ x + h[k]
    return Wt, f


@pytest.mark.parametrize("nx,nu,N,tv", [(2, 1, 20, False), (2, 2, 5, True), (3, 2, 7, True),
                                        (4, 1, 17, True), (4, 2, 16, True), (4, 1, 32, False)])
def test_row_recursion_host(nx, nu, N, tv):
    """W~ W~' against inv(H) of the explicitly condensed H at relative 1e-11
    (the bound of test_factor_identity_host: eps * cond(H) with margin) and f
    at relative 1e-12 (a few hundred roundings of 1.1e-16 along the horizon).
    Time-varying cases carry a drift."""
    rng = np.random.default_rng(100 * nx + 10 * nu + N)
    if (nx, nu, N, tv) == (2, 1, 20, False):
        A, B, Q, R, Qf = _cfg2_plant()
    else:
        A, B, Q, R, Qf = _plants(rng, nx, nu, N, tv)
    x0 = rng.normal(size=nx) * 3
    c = rng.normal(size=(N, nx)) * 0.3 if tv else None
    ref = oc.condense(A, B, Q, R, Qf, N, x0=x0, c=c)
    Hi = np.linalg.inv(ref["H"])
    Wt, f = _rows_and_f(A, B, Q, R, Qf, N, x0, c)
    assert np.array_equal(Wt, np.tril(Wt))  # rows t < j of a column are 0, L_j is lower
    errM = np.abs(Wt @ Wt.T - Hi).max() / np.abs(Hi).max()
    errf = np.abs(f - ref["f"]).max() / np.abs(ref["f"]).max()
    print(f"nx={nx} nu={nu} N={N} tv={tv}: W~W~' rel err {errM:.2e}, f rel err {errf:.2e}")
    assert errM < 1e-11
    assert errf < 1e-12


def _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv, dt=torch.float64):
    return batched.mpc_box(_t(A, dev, dt), _t(B, dev, dt), _t(Q, dev, dt), _t(R, dev, dt),
                           _t(Qf, dev, dt), N, _t(x0, dev, dt), _t(lb, dev, dt), _t(ub, dev, dt),
                           c=None if c is None else _t(c, dev, dt), tv=tv)


def _cfg2_batch(rng, batch):
    A, B, Q, R, Qf = _cfg2_plant()
    Ab = np.broadcast_to(A, (batch, 2, 2))
    Bb = np.broadcast_to(B, (batch, 2, 1))
    x0 = rng.uniform(-10, 10, (batch, 2))
    return Ab, Bb, Q, R, Qf, x0


def _case(rng, nx, nu, N, tv, drift, batch):
    """Inputs of one case; nx = 0 stands for the config-2 plant (n = 20,
    |u| <= 1, x0 ~ U(-10, 10)^2)."""
    if nx == 0:
        A, B, Q, R, Qf, x0 = _cfg2_batch(rng, batch)
        nx, n = 2, N
        lb, ub = -np.ones((batch, n)), np.ones((batch, n))
    else:
        A, B, Q, R, Qf = _plants(rng, nx, nu, N, tv, batch)
        x0 = rng.normal(size=(batch, nx)) * 3
        n = N * nu
        lb = -rng.uniform(0.2, 1.0, (batch, n))
        ub = rng.uniform(0.2, 1.0, (batch, n))
    c = rng.normal(size=(batch, N, nx)) * 0.3 if drift else None
    return A, B, Q, R, Qf, x0, lb, ub, c


def _check_vs_oracle(z, A, B, Q, R, Qf, N, x0, lb, ub, c, tol=1e-9):
    for b in range(z.shape[0]):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b], c=None if c is None else c[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], lb[b], ub[b])
        err = np.abs(z[b] - zr).max()
        assert err < tol * max(1, np.abs(zr).max()), (b, err)


# (nx, nu, N, tv, drift); nx = 0: the config-2 plant.  Qf != Q everywhere.
#   N = 1 (no off-diagonal row, one pass of the loop), nu = 1 and 2;  N = 2;
#   n = 16 (one row per lane);  n = 17 (the first second-row chain);  n = 20;
#   n = 32 full as (4,1,32) and (4,2,16);  padded states nx = 1, 3;  nu = 2
#   with nx = 3 (2 x 2 factor, padded state);  each of LTI / time-varying
#   with and without a drift.
# Only the kernels for nx <= 2 take the row form (QMpcRows, quad_box.hip);
# those for nx = 3, 4, and in fp64 those for nu = 2 with n <= 12, keep the
# two-loop setup and must behave as before.  So fp64 N = 1 and N = 2 reach the
# row form with nu = 1 only; with nu = 2 they cannot in fp64 (test_rows_fp32
# runs them in fp32).  Every other property above is also drawn with nx <= 2
# on the row form (second block): n = 32 full
# as (2,1,32) and (2,2,16), n = 24, 26 and 28 (block sizes 6 and 7 with
# padding rows), time-varying without a drift at n = 17, 21, 26 and 32, the 2 x 2
# factor at n = 16, 20 and with a padded state (nx = 1).
CASES = [(2, 1, 1, False, False), (2, 2, 1, False, True), (2, 1, 2, True, False),
         (2, 2, 2, True, True), (2, 1, 16, False, True), (2, 1, 17, True, True),
         (0, 1, 20, False, False), (0, 1, 20, False, True), (4, 1, 32, False, False),
         (4, 1, 32, True, False), (4, 2, 16, True, True), (4, 2, 16, False, True),
         (1, 1, 7, False, True), (3, 1, 12, True, False), (3, 2, 9, True, True),
         (3, 2, 9, False, False),
         (2, 1, 5, True, True), (2, 2, 8, True, True), (2, 2, 10, False, True), (1, 2, 8, False, False),
         (2, 1, 32, False, False), (2, 1, 32, True, True), (2, 2, 16, True, False),
         (2, 2, 16, False, True), (2, 1, 24, False, True), (2, 2, 14, True, True),
         (2, 1, 17, True, False), (2, 2, 13, True, False), (1, 1, 21, True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [5, 7])
@pytest.mark.parametrize("nx,nu,N,tv,drift", CASES)
def test_rows_vs_oracle(dev, nx, nu, N, tv, drift, batch):
    """Partial waves and dead groups (batch 5, 7): 1e-9 max(1, |z_ref|_inf)
    against explicit condensing + active set, every status 0."""
    rng = np.random.default_rng(2000 * batch + 131 * nx + 17 * nu + 3 * N + 2 * tv + drift)
    A, B, Q, R, Qf, x0, lb, ub, c = _case(rng, nx, nu, N, tv, drift, batch)
    z, st = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    assert (batched.status_code(st) == 0).all(), st
    _check_vs_oracle(z.cpu().numpy(), A, B, Q, R, Qf, N, x0, lb, ub, c)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,tv", [(0, 1, 20, False), (3, 2, 9, True), (4, 1, 32, False),
                                        (2, 1, 17, True), (2, 2, 13, True), (2, 1, 1, False)])
def test_rows_zero_state(dev, nx, nu, N, tv):
    """x0 = 0 without a drift: f = 0 exactly, so z = 0 in 0 iterations."""
    batch = 5
    A, B, Q, R, Qf, x0, lb, ub, _ = _case(np.random.default_rng(5), nx, nu, N, tv, False, batch)
    z, st = _solve(dev, A, B, Q, R, Qf, N, np.zeros_like(x0), lb, ub, None, tv)
    assert (batched.status_code(st) == 0).all(), st
    assert (batched.status_iters(st) == 0).all(), st
    assert float(z.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,tv,drift", [(0, 1, 20, False, True), (2, 1, 17, True, True),
                                              (3, 2, 9, False, True), (4, 2, 16, True, False),
                                              (2, 1, 17, True, False), (2, 2, 16, True, False)])
def test_rows_vs_column_construction(dev, nx, nu, N, tv, drift, monkeypatch):
    """Same inputs through the default kernel and through the
    one-QP-per-wavefront kernel (column-by-column H^{-1}, sequential adjoint)."""
    batch = 7
    A, B, Q, R, Qf, x0, lb, ub, c = _case(np.random.default_rng(78), nx, nu, N, tv, drift, batch)
    zq, sq = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    monkeypatch.setenv("MPCQP_KERNEL", "wave")
    zw, sw = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    monkeypatch.delenv("MPCQP_KERNEL")
    assert torch.equal(batched.status_code(sq), batched.status_code(sw))
    assert (batched.status_code(sq) == 0).all()
    assert float((zq - zw).abs().max()) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,tv", [(0, 1, 20, False), (2, 1, 1, False), (2, 2, 1, True),
                                        (2, 1, 2, False), (2, 2, 2, True)])
def test_rows_fp32(dev, nx, nu, N, tv):
    """fp32 with a drift: 2e-3 absolute on |u| <= 1, the tolerance of
    test_fused_factor_fp32 (config-2 plant, cond(H) ~ 6e3; the N = 1 and N = 2
    plants are better conditioned).  Every fp32 nx <= 2 kernel is on the row
    form, so this is where N = 1 and N = 2 run through it."""
    batch = 7
    rng = np.random.default_rng(9 + N)
    A, B, Q, R, Qf, x0, lb, ub, c = _case(rng, nx, nu, N, tv, True, batch)
    if nx == 0:
        x0, c = x0 * 0.3, c * 0.1
    z, st = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv, torch.float32)
    assert (batched.status_code(st) == 0).all()
    zh = z.double().cpu().numpy()
    for b in range(batch):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b], c=c[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], lb[b], ub[b])
        assert np.abs(zh[b] - zr).max() < 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,N,tv,drift", [(2, 1, 32, False, True), (2, 2, 14, True, False),
                                              (2, 1, 24, True, True)])
def test_rows_fp32_large_blocks(dev, nx, nu, N, tv, drift):
    """The fp32 row-form kernels with block sizes 6..8 (n = 24, 28, 32).  The
    free part of z solves a system in a principal block of H, so rounding the
    data and the arithmetic to fp32 moves it by c * eps32 * cond(H) * |z|_inf;
    c = 100 allows for the n = 32 terms of each sum and for the Riccati
    recursion feeding W~ (set before running the kernel)."""
    batch = 5
    rng = np.random.default_rng(300 + N)
    A, B, Q, R, Qf, x0, lb, ub, c = _case(rng, nx, nu, N, tv, drift, batch)
    z, st = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv, torch.float32)
    assert (batched.status_code(st) == 0).all()
    zh = z.double().cpu().numpy()
    eps32 = float(np.finfo(np.float32).eps)
    for b in range(batch):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b], c=None if c is None else c[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], lb[b], ub[b])
        tol = 100 * eps32 * np.linalg.cond(ref["H"]) * max(1.0, np.abs(zr).max())
        err = np.abs(zh[b] - zr).max()
        print(f"n={N * nu} b={b}: err {err:.2e} tol {tol:.2e}")
        assert err < tol
