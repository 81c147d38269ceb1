"""CPU: mpcqp_mpc_poly_loop_soft is exported and rejects bad arguments before
any launch; and, on the reference alone (tests/_poly_soft_cases.py: the QP with
explicit slacks, KKT-certified at every step), the scenarios of
tests/test_gpu_poly_soft.py are what that file claims: softened steps in every
parameter set, the exactness premise, hard-active and soft-active soft rows in
every shape and at the rebuild steps -- so that a green GPU run means
something."""
import ctypes

import numpy as np
import pytest

import _poly_loop_cases as pc
import _poly_soft_cases as sc
from model_predictive_control_amd import _native as nat


@pytest.fixture(scope="module")
def lib():
    return nat.load()


def _call(lib, *, batch=1, n=5, m=10, nbox=1, nx=2, nu=1, steps=3, ws=1, sx=2, sh=0, sigma=1):
    """mpcqp_mpc_poly_loop_soft with dummy non-null pointers (never
    dereferenced: every case here is rejected, or batch = 0, before a launch)."""
    one = ctypes.c_void_p(1)
    return lib.mpcqp_mpc_poly_loop_soft(nat.F64, batch, n, m, nbox, nx, nu, steps, 0,
                                        ctypes.c_void_p(ws) if ws else None, one, one, one, one,
                                        sx, one, one, sh, one, one, None, one,
                                        one if sigma else None, one, one, None, None, None, one,
                                        0, 0.0, None)


def test_soft_loop_symbol_and_args_rejected_without_gpu(lib):
    assert hasattr(lib, "mpcqp_mpc_poly_loop_soft") and nat.STATUS_SOFTENED == 1 << 26
    assert "mpcqp_mpc_poly_loop_soft" in nat.SIGNATURES
    assert _call(lib, m=60) == -1 and b"m_total=65" in lib.mpcqp_last_error()
    assert b"mpcqp_mpc_poly_loop_soft" in lib.mpcqp_last_error()
    assert _call(lib, m=0, nbox=0) == -1 and b"m_total=0" in lib.mpcqp_last_error()
    assert _call(lib, n=20, m=4, nu=17) == -1 and b"nu=17" in lib.mpcqp_last_error()
    assert _call(lib, nu=6) == -1                       # nu > n
    assert _call(lib, nx=17) == -1 and b"nx=17" in lib.mpcqp_last_error()
    assert _call(lib, steps=-1) == -1 and b"steps=-1" in lib.mpcqp_last_error()
    assert _call(lib, ws=0) == -1 and b"required" in lib.mpcqp_last_error()
    assert _call(lib, sx=-2) == -1 and b"negative stride" in lib.mpcqp_last_error()
    assert _call(lib, sh=-1) == -1 and b"negative stride" in lib.mpcqp_last_error()
    assert _call(lib, sigma=0) == -1 and b"sigma" in lib.mpcqp_last_error()
    assert _call(lib, batch=0) == 0


# ------------------------------------------------------------ reference only
@pytest.mark.parametrize("rho,sigma", sc.PENALTIES)
def test_reference_loss_of_feasibility_softened(rho, sigma):
    """Test 1: every step of every episode has a KKT-certified solution (the
    assertion inside SoftQP.step), and softened steps occur in the episodes
    that lose feasibility as hard problems, for every parameter set."""
    total = 0
    for N in (5, 3):
        sq, X0, ref = sc.feasibility_reference(N, rho, sigma)
        for i, (xs, zs, ys, es) in enumerate(ref):
            assert np.isfinite(xs).all()
            soft = int((es > 0).any(axis=1).sum())
            total += soft
            if i < len(X0) - 1:
                assert soft > 0, (N, i)
    print(f"({rho}, {sigma}): {total} of {5 * pc.T_EPISODE} steps softened")
    assert total > 0


def test_reference_exactness_premise():
    """Test 2: the largest |y| on a state row over the feasible session
    episodes is below rho = 2000, so that penalty is exact there."""
    for name in ("Problem", "Problem3"):
        for N in (5, 10):
            qp, refs = pc.session_reference(name, N)
            worst = 0.0
            for xs, _, _, fail in refs:
                assert fail is None
                for t in range(pc.T_EPISODE):
                    worst = max(worst, np.abs(qp.step(xs[t])[1][:qp.m]).max())
            print(f"{name} N={N}: largest state-row multiplier {worst:.0f}")
            assert worst < 2000.0


@pytest.mark.parametrize("nx,nu,N", pc.SHAPES)
def test_reference_shapes_softened_and_hard_active(nx, nu, N):
    """Test 5: every shape has a softened step and a hard-active soft row,
    with rho = 0.02; with rho = 0 it has softened steps."""
    sq, _, ref = sc.shape_soft(nx, nu, N)
    soft = hard = 0
    for xs, zs, ys, es in ref:
        sa, ha = sc.regimes(sq, ys)
        soft += int(sa.any(axis=1).sum())
        hard += int(ha.sum())
        assert np.array_equal(sa.any(axis=1), (es > 1e-12).any(axis=1))
    sq0, _, ref0 = sc.shape_soft(nx, nu, N, rho=0.0)
    soft0 = sum(int((es > 0).any(axis=1).sum()) for _, _, _, es in ref0)
    print(f"({nx}, {nu}, {N}): softened steps {soft} (rho = 0: {soft0}) of "
          f"{pc.SHAPE_B * pc.SHAPE_T}, hard-active soft rows {hard}")
    assert soft > 0 and hard > 0 and soft0 > 0


def test_reference_drift_regimes_at_rebuild():
    """Test 6: nearly every step is softened, and the steps whose active set
    the rebuild sweeps back in (63, 127, 191) carry both soft-active and
    hard-active soft rows."""
    sq, w, ref = sc.drift_soft()
    for xs, zs, ys, es in ref:
        assert int((es > 0).any(axis=1).sum()) >= 180
        sa, ha = sc.regimes(sq, ys)
        for t in (63, 127, 191):
            assert sa[t].any() and ha[t].any(), t
    print(f"drift: {int((ref[0][3] > 0).any(axis=1).sum())} of {pc.T_DRIFT} steps softened; "
          f"step 63: {int(sa[63].sum())} soft-active, {int(ha[63].sum())} hard-active")


def test_reference_config4_softened():
    """Test 7: certified at every step, with soft-active and hard-active rows."""
    sq, _, ref = sc.config4_soft()
    soft = hard = 0
    for xs, zs, ys, es in ref:
        sa, ha = sc.regimes(sq, ys)
        soft += int(sa.sum())
        hard += int(ha.sum())
    print(f"config 4: {soft} soft-active and {hard} hard-active rows")
    assert soft > 0 and hard > 0
