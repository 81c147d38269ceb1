"""The setup loop of the fused box kernel, one loop per launch-flag combination.

The row-form kernels of mpcqp_mpc_box (nx <= 2; quad_box.hip) run Riccati
stage N-1-t, free-response stage t, the columns of stage N-1-t of W~ and the
Lyapunov recursion for f in one loop over t.  Its text (mpc_setup_stage.inc)
is compiled once per combination of the wave-uniform flags "time-varying
plant" and "drift", and the kernel picks the loop in front of it; without a
drift the read-ahead of c is a constant.  The fp64 nu = 1 kernels for n >= 17
run two stages per trip and leave the last stage of an odd N behind the loop
(N = 17, 19, 21, 23, 27, 31 below).  In fp64 the kernels for n >= 13
(nu = 2: n >= 17) take that form, in fp32 all of them, so the small horizons
reach it in fp32 and run in fp64 through the one loop that tests the flags.
The arithmetic per instance is the parent's in the parent's order, so the
cases are those at which the loop itself can go wrong: the first and last
trips (N = 1, 2, 3, odd N), the padding rows n .. NV-1 of every block size,
one and two columns per stage, padded states, each of the four loops, dead
groups, and a NOT_CONVEX instance between ordinary ones.

Every case is held against explicit condensing + active set (oracle.condense,
oracle.qp) at the tolerances of test_gpu_mpc_box_rows.py: fp64 1e-9 *
max(1, |z_ref|_inf); fp32 2e-3 absolute on |u| <= 1 for the config-2 plant, and
for the random plants its 100 * eps32 * cond(H) * max(1, |z_ref|_inf).
"""
import numpy as np
import pytest
import torch

import _mpc_setup_cases as sc
from model_predictive_control_amd import batched

gpu = pytest.mark.gpu
NOT_CONVEX = 2
EPS32 = float(np.finfo(np.float32).eps)


def _t(a, dev, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _solve(dev, inp, N, tv, dt=torch.float64):
    A, B, Q, R, Qf, x0, lb, ub, c = inp
    t = lambda a: _t(a, dev, dt)  # noqa: E731
    z, st = batched.mpc_box(t(A), t(B), t(Q), t(R), t(Qf), N, t(x0), t(lb), t(ub),
                            c=None if c is None else t(c), tv=tv)
    torch.cuda.synchronize()
    return z, st


def _seed(nx, nu, N, tv, drift, batch):
    return 7000 * batch + 131 * nx + 17 * nu + 3 * N + 2 * tv + drift


def _check(dev, nx, nu, N, tv, drift, batch, fp32):
    if fp32 and nx == 0:
        inp, zr, cond = sc.case_with_reference(_seed(nx, nu, N, tv, drift, batch), nx, nu, N, tv,
                                               drift, batch, 0.3, 0.1)
    else:
        inp, zr, cond = sc.case_with_reference(_seed(nx, nu, N, tv, drift, batch), nx, nu, N, tv,
                                               drift, batch)
    z, st = _solve(dev, inp, N, tv, torch.float32 if fp32 else torch.float64)
    assert (batched.status_code(st) == 0).all(), st
    zh = z.double().cpu().numpy()
    for b in range(batch):
        scale = max(1.0, np.abs(zr[b]).max())
        if not fp32:
            tol = 1e-9 * scale
        elif nx == 0:
            tol = 2e-3
        else:
            tol = 100 * EPS32 * cond[b] * scale
        err = np.abs(zh[b] - zr[b]).max()
        print(f"nx={nx} nu={nu} N={N} tv={tv} drift={drift} fp32={fp32} b={b}: err {err:.2e} tol {tol:.2e}")
        assert err < tol, (b, err, tol)


# ------------------------------------------------------------- 1. horizons
# N = 1: one trip, forward stage 0 next to backward stage 0; N = 2; N = 3 and
# 7: odd.  On the four loops in fp32; fp64 keeps the one loop at these sizes.
@gpu
@pytest.mark.parametrize("fp32", [True, False])
@pytest.mark.parametrize("batch", [5, 7])
@pytest.mark.parametrize("nx,nu,N,tv,drift", [(2, 1, 1, False, False), (2, 2, 1, True, True),
                                              (2, 1, 2, True, False), (2, 2, 2, False, True),
                                              (1, 1, 3, False, True), (2, 2, 3, True, False),
                                              (2, 1, 7, True, True), (2, 2, 7, False, False)])
def test_setup_horizons(dev, nx, nu, N, tv, drift, batch, fp32):
    _check(dev, nx, nu, N, tv, drift, batch, fp32)


# ---------------------------------------------------------- 2. padding rows
# n = 4 BS - 1 and n = 4 BS for BS = 1 .. 8: with and without rows n .. NV-1.
# nu = 1 at every n (the config-2 plant up to n = 20, where its fp32 bound
# holds; random plants above), nu = 2 (two columns per stage) at the even ones.
PAD = [(0 if n <= 20 else 2, 1, n) for bs in range(1, 9) for n in (4 * bs - 1, 4 * bs)] + \
      [(2 - bs % 2, 2, 2 * bs) for bs in range(1, 9)]


@gpu
@pytest.mark.parametrize("fp32", [True, False])
@pytest.mark.parametrize("nx,nu,N", PAD)
def test_setup_padding_rows(dev, nx, nu, N, fp32):
    n = N * nu
    _check(dev, nx, nu, N, nx != 0 and n % 3 == 0, n % 2 == 1, 5 + 2 * (n % 2), fp32)


# ------------------------------------------------ 3. the four loops, nx, odd N
# Time-varying / LTI with and without a drift -- one compiled loop each -- at
# sizes whose fp64 kernels have the four loops: nu = 1 at n = 20, 21 (odd N,
# BS = 6) and 17, nu = 2 at n = 22 (N = 11, odd) and 32; nx = 1 and 2, and the
# config-2 plant.
FLAGS = [(2, 1, 20), (1, 1, 21), (1, 2, 11), (2, 2, 16), (2, 1, 17)]


@gpu
@pytest.mark.parametrize("batch", [5, 7])
@pytest.mark.parametrize("tv,drift", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("nx,nu,N", FLAGS)
def test_setup_flag_loops(dev, nx, nu, N, tv, drift, batch):
    _check(dev, nx, nu, N, tv, drift, batch, False)


@gpu
@pytest.mark.parametrize("drift", [False, True])
def test_setup_config2_plant(dev, drift):
    _check(dev, 0, 1, 20, False, drift, 7, False)
    _check(dev, 0, 1, 20, False, drift, 7, True)


# --------------------------------------------------------------- 4. NOT_CONVEX
@gpu
@pytest.mark.parametrize("nx,nu,N,tv", [(2, 1, 20, False), (2, 2, 12, True), (0, 1, 20, False)])
def test_setup_not_convex_between_neighbours(dev, nx, nu, N, tv):
    """R < 0 in instances 1 and 5 of 7 (a full wave, and one with a dead group):
    S_k <= 0, so their columns of W~ hold NaN.  They report NOT_CONVEX with a
    NaN z, and the others equal, bit for bit, the same instances solved in a
    batch without them."""
    batch = 7
    inp, zr, _ = sc.case_with_reference(_seed(nx, nu, N, tv, True, batch), nx, nu, N, tv, True, batch)
    A, B, Q, R, Qf, x0, lb, ub, c = inp
    Rb = np.broadcast_to(R, (batch,) + R.shape).copy()
    z0, st0 = _solve(dev, (A, B, Q, Rb, Qf, x0, lb, ub, c), N, tv)
    Rbad = Rb.copy()
    Rbad[[1, 5]] = -1e6 * np.eye(R.shape[0])
    z1, st1 = _solve(dev, (A, B, Q, Rbad, Qf, x0, lb, ub, c), N, tv)
    z0, z1, st0, st1 = z0.cpu().numpy(), z1.cpu().numpy(), st0.cpu().numpy(), st1.cpu().numpy()
    assert (st0 & 0xFF == 0).all(), st0
    for b in (1, 5):
        assert (st1[b] & 0xFF) == NOT_CONVEX and np.isnan(z1[b]).all(), (b, st1[b], z1[b])
    for b in (0, 2, 3, 4, 6):
        assert st1[b] == st0[b], (b, st1, st0)
        assert np.array_equal(z1[b].view(np.uint64), z0[b].view(np.uint64)), b
        assert np.abs(z1[b] - zr[b]).max() < 1e-9 * max(1.0, np.abs(zr[b]).max())


# ------------------------------------------ 5. against the column construction
# One case of each family above through the one-QP-per-wavefront kernel
# (column-by-column H^-1, sequential adjoint), as test_rows_vs_column_construction.
@gpu
@pytest.mark.parametrize("nx,nu,N,tv,drift", [(2, 1, 7, True, True), (2, 1, 23, False, True),
                                              (1, 2, 11, True, False), (0, 1, 20, False, False),
                                              (2, 2, 16, False, True)])
def test_setup_vs_column_construction(dev, nx, nu, N, tv, drift, monkeypatch):
    batch = 7
    inp = sc.case(78 + N, nx, nu, N, tv, drift, batch)
    zq, sq = _solve(dev, inp, N, tv)
    monkeypatch.setenv("MPCQP_KERNEL", "wave")
    zw, sw = _solve(dev, inp, N, tv)
    monkeypatch.delenv("MPCQP_KERNEL")
    assert torch.equal(batched.status_code(sq), batched.status_code(sw))
    assert (batched.status_code(sq) == 0).all()
    assert float((zq - zw).abs().max()) < 1e-9
