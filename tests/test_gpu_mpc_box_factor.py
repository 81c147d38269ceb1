"""The fused box kernel's -H^{-1} = -W S^{-1} W' construction.

mpcqp_mpc_box (four QPs per wavefront) forms H^{-1} from the Riccati pass:
H = T' diag(S_k) T with T: u -> (u_k - K_k x_k(u)), so H^{-1} = W diag(S_k^{-1}) W'
with W = T^{-1}, whose column (j, b) is a closed-loop rollout started at stage j.
The identity is restated here in NumPy and checked on the host; the kernel is
checked against the oracle (explicit condensing + active set) on every shape
at which it takes another path, and against the one-QP-per-wavefront kernel
(MPCQP_KERNEL=wave), which still builds the columns of H^{-1} one by one.
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
    """Random (marginally) stable plants and weights, as test_gpu_box.py's
    fused test draws them; batch=None gives one instance."""
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


def _w_sinv_wt(A, B, Q, R, Qf, N):
    """H^{-1} = W diag(S_k^{-1}) W' from the Riccati recursion."""
    nx, nu = B.shape[-2:]
    st = lambda M, k: M[k] if M.ndim == 3 else M  # noqa: E731
    P = Qf
    K, Acl, Si = [None] * N, [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Ak, Bk = st(A, k), st(B, k)
        S = R + Bk.T @ P @ Bk
        Si[k] = np.linalg.inv(S)
        K[k] = -Si[k] @ Bk.T @ P @ Ak
        Acl[k] = Ak + Bk @ K[k]
        P = Q + Ak.T @ P @ Ak + Ak.T @ P @ Bk @ K[k]
    n = N * nu
    W = np.zeros((n, n))
    for j in range(N):
        for b in range(nu):
            c = j * nu + b
            W[c, c] = 1.0
            x = st(B, j)[:, b]
            for k in range(j + 1, N):
                W[k * nu:(k + 1) * nu, c] = K[k] @ x
                x = Acl[k] @ x
    D = np.zeros((n, n))
    for k in range(N):
        D[k * nu:(k + 1) * nu, k * nu:(k + 1) * nu] = Si[k]
    return W @ D @ W.T


@pytest.mark.parametrize("nx,nu,N,tv", [(2, 1, 20, False), (2, 2, 5, True), (3, 2, 7, True),
                                        (4, 1, 17, True), (4, 2, 16, True)])
def test_factor_identity_host(nx, nu, N, tv):
    """W S^{-1} W' against the inverse of the explicitly condensed H, fp64 on
    the host: relative 1e-11 (eps * cond(H) ~ 1e-16 * 1e4, with margin)."""
    if (nx, nu, N, tv) == (2, 1, 20, False):
        A, B, Q, R, Qf = _cfg2_plant()
    else:
        A, B, Q, R, Qf = _plants(np.random.default_rng(100 * nx + 10 * nu + N), nx, nu, N, tv)
    H = oc.condense(A, B, Q, R, Qf, N)["H"]
    Hi = np.linalg.inv(H)
    err = np.abs(_w_sinv_wt(A, B, Q, R, Qf, N) - Hi).max() / np.abs(Hi).max()
    print(f"nx={nx} nu={nu} N={N} tv={tv}: rel err {err:.2e}, cond(H) {np.linalg.cond(H):.2e}")
    assert err < 1e-11


def _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv, dt=torch.float64):
    z, st = batched.mpc_box(_t(A, dev, dt), _t(B, dev, dt), _t(Q, dev, dt), _t(R, dev, dt),
                            _t(Qf, dev, dt), N, _t(x0, dev, dt), _t(lb, dev, dt), _t(ub, dev, dt),
                            c=None if c is None else _t(c, dev, dt), tv=tv)
    return z, st


# n = 1; n = 16 (one column per lane); n = 17 (the first second column);
# n = 20 (config-2 size); n = 32 full (nu = 1 and nu = 2); padded states
# (nx = 1, 3); 2 x 2 Cholesky scaling with a padded state and a drift
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [5, 7])
@pytest.mark.parametrize("nx,nu,N,tv", [(2, 1, 1, False), (2, 1, 16, False), (2, 1, 17, True),
                                        (2, 1, 20, False), (4, 1, 32, False), (4, 2, 16, True),
                                        (1, 1, 7, False), (3, 1, 12, False), (3, 2, 9, True)])
def test_fused_factor_vs_oracle(dev, nx, nu, N, tv, batch):
    rng = np.random.default_rng(1000 * batch + 31 * nx + 7 * nu + N)
    A, B, Q, R, Qf = _plants(rng, nx, nu, N, tv, batch)
    x0 = rng.normal(size=(batch, nx)) * 3
    c = rng.normal(size=(batch, N, nx)) * 0.3 if tv else None  # time-varying cases carry a drift
    n = N * nu
    lb = -rng.uniform(0.2, 1.0, (batch, n))
    ub = rng.uniform(0.2, 1.0, (batch, n))
    z, st = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    z = z.cpu().numpy()
    assert (batched.status_code(st) == 0).all(), st
    for b in range(batch):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b], c=None if c is None else c[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], lb[b], ub[b])
        err = np.abs(z[b] - zr).max()
        assert err < 1e-9 * max(1, np.abs(zr).max()), (b, err)


def _cfg2_batch(rng, batch):
    A, B, Q, R, Qf = _cfg2_plant()
    Ab = np.broadcast_to(A, (batch, 2, 2))
    Bb = np.broadcast_to(B, (batch, 2, 1))
    x0 = rng.uniform(-10, 10, (batch, 2))
    return Ab, Bb, Q, R, Qf, x0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n17_tv", "cfg2"])
def test_factor_vs_column_construction(dev, case, monkeypatch):
    """Same inputs through the default kernel (W S^{-1} W') and through the
    one-QP-per-wavefront kernel (column-by-column H^{-1})."""
    rng = np.random.default_rng(77)
    if case == "n17_tv":
        batch, N, tv = 7, 17, True
        A, B, Q, R, Qf = _plants(rng, 2, 1, N, tv, batch)
        x0 = rng.normal(size=(batch, 2)) * 3
        c = rng.normal(size=(batch, N, 2)) * 0.3
        lb = -rng.uniform(0.2, 1.0, (batch, N))
        ub = rng.uniform(0.2, 1.0, (batch, N))
    else:
        batch, N, tv, c = 9, 20, False, None
        A, B, Q, R, Qf, x0 = _cfg2_batch(rng, batch)
        lb, ub = -np.ones((batch, N)), np.ones((batch, N))
    zq, sq = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    monkeypatch.setenv("MPCQP_KERNEL", "wave")
    zw, sw = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, c, tv)
    monkeypatch.delenv("MPCQP_KERNEL")
    assert torch.equal(batched.status_code(sq), batched.status_code(sw))
    assert (batched.status_code(sq) == 0).all()
    assert float((zq - zw).abs().max()) < 1e-9


@pytest.mark.gpu
def test_fused_factor_fp32(dev):
    """fp32 with cond(H) ~ 6e3: 2e-3 absolute on |u| <= 1 (test_mpc_box_fp32)."""
    batch, N = 9, 20
    A, B, Q, R, Qf, x0 = _cfg2_batch(np.random.default_rng(8), batch)
    x0 = x0 * 0.3
    lb, ub = -np.ones((batch, N)), np.ones((batch, N))
    z, st = _solve(dev, A, B, Q, R, Qf, N, x0, lb, ub, None, False, torch.float32)
    z = z.double().cpu().numpy()
    assert (batched.status_code(st) == 0).all()
    for b in range(batch):
        ref = oc.condense(A[b], B[b], Q, R, Qf, N, x0=x0[b])
        zr, _, _ = oq.box_qp(ref["H"], ref["f"], -np.ones(N), np.ones(N))
        assert np.abs(z[b] - zr).max() < 2e-3
