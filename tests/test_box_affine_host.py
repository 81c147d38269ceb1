"""CPU: mpcqp_mpc_box_loop_affine is exported and rejects bad arguments before
touching the GPU, and the scenarios of tests/_box_affine_cases.py are what
tests/test_gpu_box_affine.py needs them to be, on the oracle alone: every step
KKT-certified, bounds that act and variables that stay free at every shape, a
linear term g that moves the optimum, and a setpoint that the oracle's own
loop reaches with a saturated input on the way."""
import ctypes

import numpy as np
import pytest

import _box_affine_cases as bc
from model_predictive_control_amd import _native as nat


def _call(lib, *, dtype=nat.F64, batch=4, nx=2, nu=1, N=8, steps=3, flags=0, g=1, strideG=0, w=1):
    """mpcqp_mpc_box_loop_affine with dummy non-null pointers (never
    dereferenced: every call here must fail in the argument checks, or have
    batch = 0)."""
    one = ctypes.c_void_p(1)
    opt = lambda v: one if v else None  # noqa: E731
    return lib.mpcqp_mpc_box_loop_affine(dtype, batch, nx, nu, N, steps, flags, one, 0, one, 0,
                                         one, 0, one, 0, one, nx, None, 0, None, 0, opt(g),
                                         strideG, opt(w), one, one, None, one, 0, 0.0, None)


def test_symbol_and_argument_checks():
    lib = nat.load()
    assert hasattr(lib, "mpcqp_mpc_box_loop_affine")
    err = lib.mpcqp_last_error
    assert _call(lib, batch=0) == 0
    assert _call(lib, batch=0, flags=nat.LOOP_COLD) == 0
    for bad in (1, 2, 32, nat.LOOP_COLD | 1):
        assert _call(lib, flags=bad) == -1 and b"flags" in err(), bad
    assert b"mpcqp_mpc_box_loop_affine" in err()
    assert _call(lib, dtype=7) == -1 and b"dtype" in err()
    assert _call(lib, nx=5) == -1 and b"nx=5" in err()
    assert _call(lib, N=33) == -1
    assert _call(lib, strideG=3) == -1 and b"strideG" in err()
    assert _call(lib, strideG=-8) == -1
    assert _call(lib, batch=0, strideG=8) == 0          # n = N * nu


@pytest.mark.parametrize("nx,nu,N", bc.SHAPES)
def test_scenarios_certified_active_and_free(nx, nu, N):
    """Every step of the oracle's loops is KKT-certified (asserted inside
    _box_affine_cases.step); at every shape some step has an active bound and
    some a free variable."""
    p = bc.problem(nx, nu, N)
    assert max(np.linalg.cond(d["H"]) for d in p["cd"]) <= 1e4
    act = free = False
    for i in range(bc.B):
        xs, zs = p["ref"][i]
        assert xs.shape == (bc.T + 1, nx) and zs.shape == (bc.T, N * nu)
        assert np.isfinite(xs).all() and np.isfinite(zs).all()
        on = (zs == p["lb"][i]) | (zs == p["ub"][i])
        act |= bool(on.any())
        free |= bool((~on).any())
    assert act and free


def test_linear_term_moves_the_optimum():
    """In at least half of the (instance, step) pairs the optimum with g_t
    differs from the optimum with g = 0 at the same state by more than 1e-3: a
    kernel that ignores g cannot pass the GPU tests."""
    differ = total = 0
    for nx, nu, N in bc.SHAPES:
        p = bc.problem(nx, nu, N)
        for i in range(bc.B):
            differ += int((np.abs(p["ref"][i][1] - p["z0"][i]).max(axis=1) > 1e-3).sum())
            total += bc.T
    print(f"g moves the optimum in {differ} of {total} pairs")
    assert total == len(bc.SHAPES) * bc.B * bc.T and 2 * differ >= total


def test_disturbance_moves_the_state():
    """w is small against the state but far above the tolerance of the plant
    check (1e-12): a kernel that ignores w cannot pass either."""
    for nx, nu, N in bc.SHAPES:
        p = bc.problem(nx, nu, N)
        assert 1e-3 < np.abs(p["w"]).max() < 0.5
        assert (np.abs(p["w"]).max(axis=-1) > 1e-6).all()


def test_setpoint_converges():
    """The FHC double integrator driven to (p*, 0): the input saturates in the
    first steps, and the oracle's own loop reaches the setpoint within SP_T; its
    last tracking error is the value pinned in _box_affine_cases."""
    sp = bc.setpoint()
    zs, xs = sp["zs"], sp["xs"]
    assert (np.abs(zs[:3, 0]) == 1.0).all(), zs[:6, 0]
    assert (np.abs(zs[:, 0]) < 1.0).any()
    err = np.abs(xs - sp["x_ref"][:bc.SP_T + 1]).max(axis=1)
    print(f"setpoint: |x_t - x_ref| every 5 steps {err[::5]}, last {err[-1]:.3e}")
    assert err[0] == bc.SP_PSTAR
    assert err[-1] < 1e-6 * bc.SP_PSTAR
    assert (err[-10:] < err[-11:-1]).all()               # still contracting at the end
    assert 0.5 * bc.SP_ORACLE_LAST < err[-1] <= bc.SP_ORACLE_LAST
    assert bc.SP_LAST_BOUND == 10 * bc.SP_ORACLE_LAST


def test_tracking_terms_per_instance_gam_on_cpu():
    """batched.tracking_terms with a per-instance Gam (b, N*nx, n) on CPU
    tensors against the NumPy formula per instance; a shared Gam gives what it
    gave before."""
    import torch

    from model_predictive_control_amd import batched

    nx, nu, N = 2, 2, 11
    p = bc.problem(nx, nu, N)
    T, b, n = bc.T, bc.B, N * nu
    rng = np.random.default_rng(15)
    x_ref = rng.normal(size=(b, T + N + 1, nx))
    u_ref = 0.1 * rng.normal(size=(T + N, nu))
    Gam = np.stack([d["Gam"] for d in p["cd"]])
    t = lambda v: torch.as_tensor(v, dtype=torch.float64)  # noqa: E731
    got = batched.tracking_terms({"Gam": t(Gam)}, t(p["Q"]), t(p["R"]), t(p["Qf"]), N, T, t(x_ref),
                                 t(u_ref)).numpy()
    want = np.stack([bc.tracking_g(Gam[i], p["Q"], p["R"], p["Qf"], N, T, x_ref[i], u_ref)
                     for i in range(b)], axis=1)
    assert got.shape == (T, b, n)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    g0 = batched.tracking_terms({"Gam": t(Gam[0])}, t(p["Q"]), t(p["R"]), t(p["Qf"]), N, T,
                                t(x_ref[0]), t(u_ref)).numpy()
    assert g0.shape == (T, n)
    assert np.abs(g0 - want[:, 0]).max() < 1e-12 * max(1.0, np.abs(want).max())
    with pytest.raises(ValueError):
        batched.tracking_terms({"Gam": t(Gam[:2])}, t(p["Q"]), t(p["R"]), t(p["Qf"]), N, T,
                               t(x_ref), t(u_ref))
