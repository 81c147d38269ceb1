"""CPU: mpcqp_mpc_poly_loop is exported and rejects bad arguments before any
launch; and, on the oracle alone, the scenarios of tests/test_gpu_poly_loop.py
are as rich as that file claims (active state and input rows, changing
active sets, loss of feasibility at known steps, a 200-step episode with a
non-empty active set), so that a green GPU test means something."""
import ctypes

import numpy as np
import pytest

import _poly_loop_cases as pc
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd.problems import Problem


@pytest.fixture(scope="module")
def lib():
    return nat.load()


def _call(lib, *, batch=1, n=5, m=10, nbox=1, nx=2, nu=1, steps=3, ws=1, sx=2, sh=0):
    """mpcqp_mpc_poly_loop with dummy non-null pointers (never dereferenced:
    every case here is rejected, or batch = 0, before a launch)."""
    one = ctypes.c_void_p(1)
    return lib.mpcqp_mpc_poly_loop(nat.F64, batch, n, m, nbox, nx, nu, steps, 0,
                                   ctypes.c_void_p(ws) if ws else None, one, one, one, one, sx,
                                   one, one, sh, one, one, None, one, one, None, None, one, 0, 0.0,
                                   None)


def test_poly_loop_args_rejected_without_gpu(lib):
    assert hasattr(lib, "mpcqp_mpc_poly_loop") and nat.LOOP_COLD == 16
    assert _call(lib, m=60) == -1 and b"m_total=65" in lib.mpcqp_last_error()
    assert _call(lib, m=0, nbox=0) == -1 and b"m_total=0" in lib.mpcqp_last_error()
    assert _call(lib, n=20, m=4, nu=17) == -1 and b"nu=17" in lib.mpcqp_last_error()
    assert _call(lib, nu=6) == -1                       # nu > n
    assert _call(lib, nx=17) == -1 and b"nx=17" in lib.mpcqp_last_error()
    assert _call(lib, steps=-1) == -1 and b"steps=-1" in lib.mpcqp_last_error()
    assert _call(lib, ws=0) == -1 and b"required" in lib.mpcqp_last_error()
    assert _call(lib, sx=-2) == -1 and b"negative stride" in lib.mpcqp_last_error()
    assert _call(lib, sh=-1) == -1 and b"negative stride" in lib.mpcqp_last_error()
    assert _call(lib, batch=0) == 0


# ------------------------------------------------------------ reference only
def _acts(name, N):
    return [r[2] for r in pc.session_reference(name, N)[1]]


def test_reference_session_scenarios_are_rich():
    """Session-2 Problem, Qf = Q, T = 12: the active sets the claims of the GPU
    file rest on, and every step feasible for both problems and horizons."""
    for name in ("Problem", "Problem3"):
        for N in (5, 10):
            for x0, r in zip(pc.X0_SESSION, pc.session_reference(name, N)[1]):
                assert r[3] is None, (name, N, x0, r[3])
    a5, a10 = _acts("Problem", 5), _acts("Problem", 10)
    m5 = 10                                              # state rows of N = 5
    both = [(a[:m5] > 0).any() and (a[m5:] > 0).any() for a in a5[2]]          # x0 = (-50, 20)
    assert any(both)
    run = best = 0
    for a in a5[1]:                                      # x0 = (-100, 25)
        hit = (a[:m5] > 0).sum() == 4 and (a[m5:] > 0).sum() == 1
        run = run + 1 if hit else 0
        best = max(best, run)
    assert best >= 7, best
    assert max((a[20:] > 0).sum() for a in a10[5]) == 10  # x0 = (0.5, -19), N = 10
    differ = total = 0
    for acts in a5 + a10:
        for t in range(1, pc.T_EPISODE):
            differ += int((acts[t] != acts[t - 1]).any())
            total += 1
    print(f"active set differs from the previous step's in {differ} of {total} pairs")
    assert total == 2 * len(pc.X0_SESSION) * (pc.T_EPISODE - 1) and 2 * differ >= total


@pytest.mark.parametrize("N,x0,fail", pc.INFEASIBLE_CASES)
def test_reference_loss_of_feasibility(N, x0, fail):
    """Problem(u_min=-2.0): the oracle's loop is KKT-certified up to the step
    before `fail` and its QP is empty at `fail`, also with every state bound
    relaxed by 1e-6."""
    qp = pc.infeasible_qp(N)
    xs, _, _, f = qp.host_loop(np.array(x0), pc.T_EPISODE)
    assert f == fail
    with pytest.raises(ValueError, match="infeasible"):
        qp.step(xs[fail], relax=1e-6)
    assert qp.host_loop(np.array(pc.FEASIBLE_NEIGHBOUR), pc.T_EPISODE)[3] is None


def test_reference_drift_scenario():
    """3f: feasible at all 200 steps, the active set non-empty in >= 190."""
    _, _, ref = pc.drift_reference()
    for xs, zs, acts, fail in ref:
        assert fail is None
        nonempty = int((acts > 0).any(axis=1).sum())
        changes = int((acts[1:] != acts[:-1]).any(axis=1).sum())
        print(f"drift: {nonempty} steps with an active row, {changes} set changes")
        assert nonempty >= 190


@pytest.mark.parametrize("nx,nu,N", pc.SHAPES)
def test_reference_shapes_feasible_and_active(nx, nu, N):
    """Every shape of the BS table: m_total as listed, every instance feasible
    at every step, a state row active somewhere."""
    p = pc.shape_problem(nx, nu, N)
    qp = p["qp"]
    assert qp.mt == N * (nx + nu) and (qp.mt + 7) // 8 == pc.SHAPES.index((nx, nu, N)) + 1
    assert np.abs(np.linalg.eigvals(qp.A)).max() <= 1.02 + 1e-12
    state = inp = 0
    for xs, zs, acts, fail in p["ref"]:
        assert fail is None
        state += int((acts[:, :qp.m] > 0).sum())
        inp += int((acts[:, qp.m:] > 0).sum())
    print(f"active: {state} state rows, {inp} input rows")
    assert state > 0, (state, inp)


def test_reference_config4_feasible_and_active():
    p = pc.config4_problem()
    assert p["qp"].mt == 40 and p["qp"].n == 200
    for xs, zs, acts, fail in p["ref"]:
        assert fail is None and (acts > 0).any()


def test_problem_defaults_are_session2():
    pr = Problem()
    assert (pr.p_max, pr.v_min, pr.v_max, pr.u_min, pr.u_max, pr.N) == (1.0, -20, 25.0, -20.0, 10.0, 5)
