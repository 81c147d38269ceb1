"""The fused MPC step (mpcqp_mpc_box) off the easy path: status codes and
their isolation inside a wavefront, max_iter, every kind of bound, the input
forms of the plant, and fp32 off the config-2 shape.

Every case runs through both kernels -- mpc_group_kernel (four QPs per
wavefront, the default) and mpc_box_kernel (one QP per wavefront,
MPCQP_KERNEL=wave) -- which must report the same status codes; both are held
to the oracle (explicit condensing, oracle/condense.py, + primal active set,
oracle/qp.py) at 1e-9 * max(1, |z_ref|_inf) in fp64.
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import condense as oc
from oracle import qp as oq
from oracle import session1 as s1
from test_gpu_mpc_box_factor import _cfg2_plant, _plants, _t

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPS32 = float(np.finfo(np.float32).eps)
PATHS = ("group", "wave")

# (nx, nu, N, tv): config-2 size; padded states (nx = 1, 3); n = 18 and 32 at
# nu = 2; n = 32 at nu = 1; a two-stage horizon
SHAPES = [(2, 1, 20, False), (1, 1, 7, False), (3, 1, 12, True), (2, 2, 9, True),
          (4, 2, 16, True), (4, 1, 32, False), (3, 2, 2, True)]


def _seed(nx, nu, N, extra=0):
    return 100000 * extra + 1000 * nx + 100 * nu + N


def _fused(dev, monkeypatch, A, B, Q, R, Qf, N, x0, lb, ub, c=None, tv=False, dt=torch.float64,
           max_iter=0):
    """The same call through both kernels: {path: (z, code, iters)} as NumPy
    arrays; the two paths must agree on every status code."""
    t = lambda a: a if (a is None or isinstance(a, float)) else _t(a, dev, dt)  # noqa: E731
    out = {}
    for path in PATHS:
        if path == "wave":
            monkeypatch.setenv("MPCQP_KERNEL", "wave")
        else:
            monkeypatch.delenv("MPCQP_KERNEL", raising=False)
        z, st = batched.mpc_box(t(A), t(B), t(Q), t(R), t(Qf), N, t(x0), t(lb), t(ub), c=t(c),
                                tv=tv, max_iter=max_iter)
        torch.cuda.synchronize()
        out[path] = (z.double().cpu().numpy(), batched.status_code(st).cpu().numpy(),
                     batched.status_iters(st).cpu().numpy())
    monkeypatch.delenv("MPCQP_KERNEL", raising=False)
    assert out["group"][1].tolist() == out["wave"][1].tolist(), (out["group"][1], out["wave"][1])
    return out


def _inst(M, b, base):
    """Instance b of an input that is shared (ndim == base) or batched."""
    return None if M is None else (M if np.ndim(M) <= base else M[b])


def _oracle(A, B, Q, R, Qf, N, x0, lb, ub, c, tv, b):
    """(z_ref, H, f, lb_b, ub_b) of instance b, KKT-certified."""
    pb = 3 if tv else 2
    ref = oc.condense(_inst(A, b, pb), _inst(B, b, pb), _inst(Q, b, 2), _inst(R, b, 2),
                      _inst(Qf, b, 2), N, x0=_inst(x0, b, 1), c=_inst(c, b, 2))
    n = ref["f"].size
    lbb = None if lb is None else np.broadcast_to(_inst(np.asarray(lb, float), b, 1), (n,))
    ubb = None if ub is None else np.broadcast_to(_inst(np.asarray(ub, float), b, 1), (n,))
    zr, _, _ = oq.box_qp(ref["H"], ref["f"], lbb, ubb)
    assert oq.kkt_box(ref["H"], ref["f"], lbb, ubb, zr) < 1e-9 * max(1, np.abs(ref["f"]).max())
    return zr, ref["H"], ref["f"], lbb, ubb


def _n_active(zr, lbb, ubb):
    at = np.zeros(zr.size, bool)
    if lbb is not None:
        at |= zr == lbb
    if ubb is not None:
        at |= zr == ubb
    return int(at.sum())


def _check_vs_oracle(out, refs, which=None, tol=None):
    """Both paths against the per-instance oracle solutions refs[b] (status 0)."""
    for path in PATHS:
        z, code, _ = out[path]
        for b, zr in enumerate(refs):
            if which is not None and b not in which:
                continue
            assert code[b] == 0, (path, b, code)
            err = np.abs(z[b] - zr).max()
            bound = (TOL if tol is None else tol[b]) * max(1, np.abs(zr).max())
            print(f"{path} b={b}: err {err:.2e} bound {bound:.2e}")
            assert err < bound, (path, b, err, bound)


def _tight_problem(nx, nu, N, tv, batch, extra=0):
    """The cases of test_fused_factor_vs_oracle with tighter bounds: most
    instances end with active bounds (asserted on the oracle by the callers)."""
    rng = np.random.default_rng(_seed(nx, nu, N, extra))
    A, B, Q, R, Qf = _plants(rng, nx, nu, N, tv, batch)
    x0 = rng.normal(size=(batch, nx)) * 3
    c = rng.normal(size=(batch, N, nx)) * 0.3 if tv else None
    n = N * nu
    lb = -rng.uniform(0.05, 0.4, (batch, n))
    ub = rng.uniform(0.05, 0.4, (batch, n))
    return dict(A=A, B=B, Q=Q, R=R, Qf=Qf, N=N, x0=x0, lb=lb, ub=ub, c=c, tv=tv), rng


def _refs(p, batch):
    return [_oracle(p["A"], p["B"], p["Q"], p["R"], p["Qf"], p["N"], p["x0"], p["lb"], p["ub"],
                    p["c"], p["tv"], b) for b in range(batch)]


# ---------------------------------------------------------------- a. statuses
def _last_stage_pivots(B, Qf, R, tv):
    """Pivots of S_{N-1} = R + B' Qf B in elimination order (the first Riccati
    stage of the kernels)."""
    Bk = B[-1] if tv else B
    S = R + Bk.T @ Qf @ Bk
    if S.shape[0] == 1:
        return [S[0, 0]]
    return [S[0, 0], S[1, 1] - S[0, 1] ** 2 / S[0, 0]]


def _status_problem(nx, nu, N, tv, batch=6):
    """Healthy per-instance problems (own Q, R, Qf per instance) and the four
    defects as functions that spoil one instance in place."""
    # seed: one at which the indefinite R below has the pivots asked for
    p, rng = _tight_problem(nx, nu, N, tv, batch, extra=2)
    s = 1.0 + 0.1 * np.arange(batch)
    p["Q"] = p["Q"][None] * s[:, None, None]
    p["R"] = p["R"][None] * (2.0 - s)[:, None, None]
    p["Qf"] = 3 * p["Q"]
    n = N * nu

    def nan_A(i):
        if tv:
            p["A"][i, N - 2, nx - 1, 0] = np.nan   # a late stage: the strided stage-in loop
            assert (N - 2) * nx * nx >= 16
        else:
            p["A"][i, nx - 1, 0] = np.nan

    def empty_box(i):
        p["lb"][i, n // 2] = p["ub"][i, n // 2] + 0.5

    def indefinite_R(i):
        p["R"][i] = np.diag([0.5, -50.0]) if nu == 2 else np.array([[-50.0]])
        piv = _last_stage_pivots(p["B"][i], p["Qf"][i], p["R"][i], tv)
        assert piv[-1] < 0 and all(v > 0 for v in piv[:-1]), piv
        H = oc.condense(p["A"][i], p["B"][i], p["Q"][i], p["R"][i], p["Qf"][i], N)["H"]
        assert np.linalg.eigvalsh(H).min() < 0

    def nan_x0(i):
        p["x0"][i, 0] = np.nan

    return p, dict(nan_A=nan_A, empty_box=empty_box, indefinite_R=indefinite_R, nan_x0=nan_x0)


def _check_statuses(out, p, expect, dt_tol=None):
    batch = len(expect)
    good = [b for b in range(batch) if expect[b] == 0]
    refs = [_oracle(p["A"], p["B"], p["Q"], p["R"], p["Qf"], p["N"], p["x0"], p["lb"], p["ub"],
                    p["c"], p["tv"], b) if b in good else None for b in range(batch)]
    for path in PATHS:
        z, code, _ = out[path]
        assert code.tolist() == list(expect), (path, code)
        for b in range(batch):
            if b in good:
                assert np.isfinite(z[b]).all(), (path, b)
            else:
                assert np.isnan(z[b]).all(), (path, b, z[b])
    tol = None if dt_tol is None else {b: dt_tol(refs[b][1]) for b in good}
    _check_vs_oracle(out, [r[0] if r is not None else None for r in refs], which=good, tol=tol)


STATUS_SHAPES = [(2, 1, 20, False), (4, 2, 16, True)]


@pytest.mark.parametrize("nx,nu,N,tv", STATUS_SHAPES)
def test_statuses_and_isolation(dev, monkeypatch, nx, nu, N, tv):
    """One full wavefront plus a half-empty one: NaN in A, an empty box, an
    indefinite R and a NaN in x0 give 4, 3, 2, 4 and an all-NaN z; the healthy
    instances next to them equal the oracle."""
    p, spoil = _status_problem(nx, nu, N, tv)
    spoil["nan_A"](1)
    spoil["empty_box"](2)
    spoil["indefinite_R"](3)
    spoil["nan_x0"](4)
    out = _fused(dev, monkeypatch, **p)
    _check_statuses(out, p, [0, 4, 3, 2, 4, 0])


@pytest.mark.parametrize("defect,code", [("nan_A", 4), ("empty_box", 3), ("indefinite_R", 2),
                                         ("nan_x0", 4)])
def test_status_in_last_lane_group(dev, monkeypatch, defect, code):
    """The bad instance in lane group 3 of the first wavefront, healthy ones
    in groups 0-2 and in the next wavefront."""
    p, spoil = _status_problem(4, 2, 16, True)
    spoil[defect](3)
    out = _fused(dev, monkeypatch, **p)
    _check_statuses(out, p, [0, 0, 0, code, 0, 0])


def test_status_precedence(dev, monkeypatch):
    """NONFINITE over INFEASIBLE over NOT_CONVEX (as box_quad_kernel), the
    same on both paths."""
    p, spoil = _status_problem(4, 2, 16, True)
    spoil["indefinite_R"](1)
    spoil["empty_box"](1)
    spoil["nan_x0"](2)
    spoil["empty_box"](2)
    spoil["indefinite_R"](4)
    spoil["nan_A"](4)
    spoil["empty_box"](4)
    out = _fused(dev, monkeypatch, **p)
    _check_statuses(out, p, [0, 3, 4, 0, 4, 0])


def test_statuses_fp32(dev, monkeypatch):
    """The status test in fp32 (healthy instances at the fp32 tolerance)."""
    nx, nu, N, tv = 4, 2, 16, True
    p, spoil = _status_problem(nx, nu, N, tv)
    spoil["nan_A"](1)
    spoil["empty_box"](2)
    spoil["indefinite_R"](3)
    spoil["nan_x0"](4)
    out = _fused(dev, monkeypatch, dt=torch.float32, **p)
    q = dict(p)
    q["A"] = p["A"].astype(np.float32).astype(np.float64)
    q["B"] = p["B"].astype(np.float32).astype(np.float64)
    _check_statuses(out, q, [0, 4, 3, 2, 4, 0], dt_tol=_tol32)


# ---------------------------------------------------------------- b. MAXITER
def test_max_iter(dev, monkeypatch):
    """Config-2 plant from x0 = (8, -3) (six active bounds) and neighbours of
    it with at least three: a dual active set adds one bound per iteration, so
    max_iter = 2 must end in MAXITER -- with a finite z inside the box -- and
    the same batch at the default max_iter is optimal."""
    A, B, Q, R, Qf = _cfg2_plant()
    N = 20
    x0 = np.array([8.0, -3.0]) * np.array([1.0, -1.0, 0.9, 1.1, -0.95, 1.2])[:, None]
    batch = x0.shape[0]
    Ab, Bb = np.broadcast_to(A, (batch, 2, 2)), np.broadcast_to(B, (batch, 2, 1))
    refs = [_oracle(Ab, Bb, Q, R, Qf, N, x0, -1.0, 1.0, None, False, b) for b in range(batch)]
    nact = [_n_active(r[0], r[3], r[4]) for r in refs]
    assert nact[0] == 6 and min(nact) >= 3, nact
    out = _fused(dev, monkeypatch, Ab, Bb, Q, R, Qf, N, x0, -1.0, 1.0, max_iter=2)
    for path in PATHS:
        z, code, iters = out[path]
        assert (code == 1).all(), (path, code)
        assert (iters <= 3).all(), (path, iters)
        assert np.isfinite(z).all() and (z >= -1.0).all() and (z <= 1.0).all(), path
    out = _fused(dev, monkeypatch, Ab, Bb, Q, R, Qf, N, x0, -1.0, 1.0)
    _check_vs_oracle(out, [r[0] for r in refs])


# ----------------------------------------------------------------- c. bounds
def _bounds(kind, p, rng, batch):
    """Replace p's bounds in place by those of `kind`."""
    n = p["N"] * p["B"].shape[-1]
    lb, ub = p["lb"], p["ub"]
    if kind == "none":
        p["lb"] = p["ub"] = None
    elif kind == "lb_only":              # of either sign: active whatever the sign of x0
        p["lb"] = lb * rng.choice([-1.0, 1.0], (batch, n))
        p["ub"] = None
    elif kind == "ub_only":
        p["ub"] = ub * rng.choice([-1.0, 1.0], (batch, n))
        p["lb"] = None
    elif kind == "inf_entries":          # as test_gpu_box._random_box_problems
        lb[rng.random((batch, n)) < 0.15] = -np.inf
        ub[rng.random((batch, n)) < 0.15] = np.inf
    elif kind == "fixed_10pct":
        fx = rng.random((batch, n)) < 0.10
        fx[0, 0] = True
        lb[fx] = ub[fx] = rng.uniform(-0.2, 0.2, (batch, n))[fx]
    elif kind == "all_fixed":
        lb[:] = rng.uniform(-0.4, 0.4, (batch, n))
        ub[:] = lb
    elif kind == "wide":
        lb[:] = -1e6
        ub[:] = 1e6
    elif kind == "tight_all_active":
        lb[:] = -rng.uniform(0.05, 0.2, (batch, n))
        ub[:] = rng.uniform(0.05, 0.2, (batch, n))
    else:
        raise AssertionError(kind)


BOUND_KINDS = ["none", "lb_only", "ub_only", "inf_entries", "fixed_10pct", "all_fixed", "wide",
               "tight_all_active"]


@pytest.mark.parametrize("kind", BOUND_KINDS)
@pytest.mark.parametrize("nx,nu,N,tv", SHAPES)
def test_bounds(dev, monkeypatch, nx, nu, N, tv, kind):
    batch = 5
    p, rng = _tight_problem(nx, nu, N, tv, batch, extra=6)
    _bounds(kind, p, rng, batch)
    n = N * nu
    if kind == "tight_all_active":
        # scale x0 up until the oracle has every bound of every instance active
        for _ in range(40):
            refs = _refs(p, batch)
            if all(_n_active(r[0], r[3], r[4]) == n for r in refs):
                break
            p["x0"] = p["x0"] * 2
    refs = _refs(p, batch)
    nact = [_n_active(r[0], r[3], r[4]) for r in refs]
    print(f"{kind} {nx, nu, N, tv}: active bounds per instance {nact} of {n}")
    if kind in ("none", "wide"):
        assert nact == [0] * batch
        for r in refs:
            assert np.abs(r[0] + np.linalg.solve(r[1], r[2])).max() < 1e-10 * max(1, np.abs(r[0]).max())
    elif kind in ("all_fixed", "tight_all_active"):
        assert nact == [n] * batch
    else:
        assert sum(k > 0 for k in nact) > batch // 2, nact    # most instances have active bounds
    out = _fused(dev, monkeypatch, **p)
    _check_vs_oracle(out, [r[0] for r in refs])
    for path in PATHS:
        z, code, iters = out[path]
        if kind == "none":
            assert (iters == 0).all(), (path, iters)
        if kind == "all_fixed":
            assert np.array_equal(z, p["lb"]), path    # bitwise


def test_unconstrained_is_riccati_feedback(dev, monkeypatch, golden):
    """No bounds on the golden session-1 plant: z is the closed-loop rollout of
    the reference's Riccati gains (as test_condense_known_answer_riccati)."""
    g = golden("session1.npz")
    A, B, Q, R, Pf = g["fhc_A"], g["fhc_B"], g["fhc_Q"], g["fhc_R"].reshape(1, 1), g["fhc_Pf"]
    N, K = 10, g["fhc_K_N10"]
    x0 = g["fhc_x0"].ravel() * np.array([1.0, -0.5, 0.1, 2.0, -1.0])[:, None]
    batch = x0.shape[0]
    Ab, Bb = np.broadcast_to(A, (batch, 2, 2)), np.broadcast_to(B, (batch, 2, 1))
    out = _fused(dev, monkeypatch, Ab, Bb, Q, R, Pf, N, x0, None, None)
    for path in PATHS:
        z, code, iters = out[path]
        assert (code == 0).all() and (iters == 0).all(), (path, code, iters)
        for b in range(batch):
            x = x0[b]
            for k in range(N):
                u = K[k] @ x
                assert abs(u[0] - z[b, k]) < 1e-10, (path, b, k)
                x = A @ x + B @ u


# ----------------------------------------------------------------- d. inputs
@pytest.mark.parametrize("per_instance_c", [False, True])
@pytest.mark.parametrize("with_x0", [True, False])
def test_lti_plant_with_drift(dev, monkeypatch, per_instance_c, with_x0):
    """tv = False with a drift c, shared (N, nx) and per instance (b, N, nx);
    x0 = None (the origin) with a drift."""
    nx, nu, N, batch = 3, 2, 8, 6
    p, rng = _tight_problem(nx, nu, N, False, batch, extra=3)
    p["c"] = rng.normal(size=(batch, N, nx) if per_instance_c else (N, nx)) * 0.5
    if not with_x0:
        p["x0"] = None
    refs = _refs(p, batch)
    assert sum(_n_active(r[0], r[3], r[4]) > 0 for r in refs) > batch // 2
    out = _fused(dev, monkeypatch, **p)
    _check_vs_oracle(out, [r[0] for r in refs])


def test_shared_and_broadcast_inputs_bitwise(dev, monkeypatch):
    """Shared (stride-0) scalar bounds against the same bounds per instance,
    and a shared plant and weights against the same ones broadcast to the
    batch: the kernels do the same arithmetic, so z is bitwise equal."""
    nx, nu, N, batch = 4, 2, 12, 7
    rng = np.random.default_rng(_seed(nx, nu, N, 4))
    A, B, Q, R, Qf = _plants(rng, nx, nu, N, True)           # one instance
    x0 = rng.normal(size=(batch, nx)) * 3
    c = rng.normal(size=(N, nx)) * 0.3
    n = N * nu
    bc = lambda M: np.broadcast_to(M, (batch,) + M.shape)    # noqa: E731
    shared = _fused(dev, monkeypatch, A, B, Q, R, Qf, N, x0, -0.3, 0.25, c=c, tv=True)
    per = _fused(dev, monkeypatch, bc(A), bc(B), bc(Q), bc(R), bc(Qf), N, x0,
                 np.full((batch, n), -0.3), np.full((batch, n), 0.25), c=bc(c), tv=True)
    mixed = _fused(dev, monkeypatch, bc(A), bc(B), Q, bc(R), Qf, N, x0, np.full(n, -0.3), 0.25,
                   c=c, tv=True)
    refs = [_oracle(A, B, Q, R, Qf, N, x0, -0.3, 0.25, c, True, b) for b in range(batch)]
    assert sum(_n_active(r[0], r[3], r[4]) > 0 for r in refs) > batch // 2
    _check_vs_oracle(shared, [r[0] for r in refs])
    for path in PATHS:
        for other in (per, mixed):
            assert np.array_equal(shared[path][0], other[path][0]), path
            assert np.array_equal(shared[path][1], other[path][1]), path
            assert np.array_equal(shared[path][2], other[path][2]), path


# ------------------------------------------------------------------- e. fp32
def _tol32(H):
    """Relative fp32 tolerance: 2e-4 (test_box_fp32, cond 1e2) up to
    3 * eps32 * cond(H) (test_mpc_box_fp32: 2e-3 at cond 6e3), cond(H) <= 1e4."""
    cond = np.linalg.cond(H)
    assert cond <= 1e4, cond
    return max(2e-4, 3 * EPS32 * cond)


@pytest.mark.parametrize("nx,nu,N,tv", SHAPES)
def test_fp32(dev, monkeypatch, nx, nu, N, tv):
    """fp32 off the config-2 shape against the fp64 oracle on the fp32-rounded
    plant (as test_condense_fp32)."""
    batch = 5
    p, _ = _tight_problem(nx, nu, N, tv, batch, extra=5)
    q = dict(p)
    q["A"] = p["A"].astype(np.float32).astype(np.float64)
    q["B"] = p["B"].astype(np.float32).astype(np.float64)
    refs = _refs(q, batch)
    assert sum(_n_active(r[0], r[3], r[4]) > 0 for r in refs) > batch // 2
    tol = [_tol32(r[1]) for r in refs]
    print("cond(H):", [f"{np.linalg.cond(r[1]):.1e}" for r in refs])
    out = _fused(dev, monkeypatch, dt=torch.float32, **p)
    _check_vs_oracle(out, [r[0] for r in refs], tol=tol)
