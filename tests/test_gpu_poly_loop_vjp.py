"""GPU: the adjoint of the one-launch polytope MPC loop (mpcqp_mpc_poly_loop_vjp)
against the NumPy recursion of tests/_poly_loop_vjp_cases.py evaluated on the
device's own xs, zs, ys; its identity with mpcqp_poly_solve_vjp on one step and
with mpcqp_mpc_box_loop_vjp on a box-only problem; its NULL arguments and status
rules; and the autograd functions built on it (poly_loop_diff,
mpc_poly_loop_diff).

Errors are max|device - reference| / (1 + max|reference|) per output array (gx0,
ghl, ghu, geps, gf, gw and the shared gH, gF, gG, gE, gA, gB), as in
tests/test_gpu_poly_vjp.py.  Tolerances: ten times the largest such error
measured over test_kernel_vs_recursion (each case prints its own); the factor 10
is the project's margin for another summation order.  A fp64 worst above 1e-9
or a fp32 worst above 1e-2 would be a finding, not a tolerance.
  fp64  measured 1.244e-12 (the session problem at N = 10, whose H is
        ill-conditioned; 1.5e-13 at (2, 1, 17), below 6e-14 everywhere else,
        3.2e-14 at config 4): the tolerance 1.244e-11 is two decades under the
        ceiling;
  fp32  measured 8.100e-4 (also the session problem at N = 10; at most 4.4e-5
        everywhere else), against the fp64 recursion on fp32-rounded data and
        the device's own fp32 xs, zs, ys: tolerance 8.1e-3, under the 1e-2 above
        which the result would be a finding.
The comparison with mpcqp_mpc_box_loop_vjp adds that kernel's own tolerance
against its closed form (tests/test_gpu_box_loop_vjp.py, 1.088e-13).
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _poly_loop_cases as lc
import _poly_loop_vjp_cases as lv
import _poly_vjp_cases as pv
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import autograd as ag
from model_predictive_control_amd import batched, poly_diff
from model_predictive_control_amd.problems import Problem

pytestmark = pytest.mark.gpu

MEASURED_F64 = 1.244e-12
MEASURED_F32 = 8.100e-4
BOX_LOOP_VJP_TOL_F64 = 1.088e-13   # TOL_F64 of tests/test_gpu_box_loop_vjp.py
TOL = {torch.float64: 10 * MEASURED_F64, torch.float32: 10 * MEASURED_F32}
CEILING_F64 = 1e-9
FINDING_F32 = 1e-2
F64, F32 = torch.float64, torch.float32
OUTS = poly_diff.LOOP_VJP_OUTPUTS
SHARED = poly_diff.LOOP_SHARED
OPT, MAXIT, NOTCVX, INFEAS, NONFIN = 0, 1, 2, 3, 4
DT = pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])


def _t(a, dev, dt=F64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _np(t):
    return t.double().cpu().numpy()


def _rel(got, ref):
    return float(np.abs(got - ref).max() / (1 + np.abs(ref).max())) if ref.size else 0.0


def _rounded(a, dt):
    return a if dt == F64 or a is None else np.asarray(a, np.float32).astype(np.float64)


def _rounded_qp(q, dt):
    """The LoopQP whose data are those the device sees in dtype dt."""
    if dt == F64:
        return q
    r = lambda a: _rounded(a, dt)  # noqa: E731
    return lc.LoopQP(r(q.H), r(q.F), r(q.G) if q.m else None, r(q.E), r(q.hl), r(q.hu),
                     r(q.lbz) if q.nbox else None, r(q.ubz) if q.nbox else None, r(q.A), r(q.B))


def _device_qp(q, dev, dt=F64):
    return batched.PolyQP(_t(pv.pack_lower(q.H), dev, dt), _t(q.G, dev, dt) if q.m else None,
                          _t(q.F, dev, dt), _t(q.lbz, dev, dt) if q.nbox else None,
                          _t(q.ubz, dev, dt) if q.nbox else None)


def _forward(q, dq, x0, T, dev, dt=F64, w=None, g=None, e=None, **kw):
    """PolyQP.loop with plans and multipliers; the operands of the plant as tensors."""
    A, B, E = _t(q.A, dev, dt), _t(q.B, dev, dt), _t(q.E, dev, dt)
    o = dq.loop(A, B, _t(x0, dev, dt), T, _t(q.hl, dev, dt) if q.m else None,
                _t(q.hu, dev, dt) if q.m else None, E, _t(w, dev, dt), plans=True, multipliers=True,
                g=_t(g, dev, dt), e=_t(e, dev, dt), **kw)
    return o, (A, B, E)


def _raw(dq, A, B, E, ys, status, gxs=None, gus=None, gzs=None, gys=None, outs=OUTS,
         scratch="alloc", steps=None, batch=None):
    """mpcqp_mpc_poly_loop_vjp as it is: only the outputs in ``outs`` passed (the
    rest NULL), pre-filled with NaN / -1 so that an entry the kernel leaves out
    shows."""
    T = ys.shape[0] if steps is None else steps
    batch = ys.shape[1] if batch is None else batch
    dt, dev = dq.dtype, A.device
    nu = B.shape[1]
    shape = dict(gx0=(batch, dq.nx), ghl=(batch, dq.mt), ghu=(batch, dq.mt), geps=(T, batch, dq.mt),
                 gf=(T, batch, dq.n), gw=(T, batch, dq.nx))
    o = {k: torch.full(shape[k], float("nan"), dtype=dt, device=dev) for k in outs}
    o["vstatus"] = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    if isinstance(scratch, str):
        nb = poly_diff.loop_scratch_bytes(dq, batch, T) if gzs is not None else 0
        scratch = torch.empty((nb,), dtype=torch.uint8, device=dev) if nb else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = nat.load().mpcqp_mpc_poly_loop_vjp(
        nat.F64 if dt == F64 else nat.F32, batch, dq.n, dq.m, dq.nbox, dq.nx, nu, T, p(dq.ws), p(E),
        p(A), p(B), p(ys), p(status), p(gxs), p(gus), p(gzs), p(gys), *(p(o.get(k)) for k in OUTS),
        p(o["vstatus"]), p(scratch), 0 if scratch is None else scratch.numel(),
        torch.cuda.current_stream().cuda_stream)
    nat.check(rc, "mpcqp_mpc_poly_loop_vjp")
    torch.cuda.synchronize()
    return o


def _upstream(q, T, batch, dev, dt, seed=0):
    """(numpy, dtype-rounded; device tensors) of the four upstream gradients."""
    ups = [_rounded(a, dt) for a in lv.upstream(T, q.nx, q.nu, q.n, q.mt, seed, batch)]
    return ups, [_t(a, dev, dt) for a in ups]


def _case_error(q, x0, T, dev, dt, w=None, g=None, e=None, sets=None):
    """Forward on the device, adjoint on the device's ys, the recursion on the
    same (dtype-rounded) data and the device's xs, zs, ys.  ``sets``: the
    oracle's row states (b, T, mt) in 0 / 1 / 2, compared in fp64.  Returns the
    worst error over the outputs and the shared gradients."""
    qr = _rounded_qp(q, dt)
    dq = _device_qp(q, dev, dt)
    batch = x0.shape[0]
    o, (A, B, E) = _forward(q, dq, x0, T, dev, dt, w=w, g=g, e=e)
    assert (batched.status_code(o["status"]) == OPT).all(), o["status"]
    ups, dups = _upstream(q, T, batch, dev, dt)
    r = _raw(dq, A, B, E, o["ys"], o["status"], *dups)
    assert (r["vstatus"] == OPT).all(), r["vstatus"]
    s = poly_diff.loop_shared_grads(dq, o["xs"], o["us"], o["zs"], o["ys"], r["gf"], r["geps"],
                                    r["gw"], r["vstatus"])
    xs, zs, ys = _np(o["xs"]), _np(o["zs"]), _np(o["ys"])
    assert torch.equal(o["us"], o["zs"][:, :, :q.nu])
    total = {}
    worst = 0.0
    for i in range(batch):
        if dt == F64 and sets is not None:
            assert (np.sign(ys[:, i]) == np.array([0, -1, 1])[sets[i][:T]]).all(), i
        ref = lv.recursion(qr, xs[:, i], zs[:, i], ys[:, i], *(u[:, i] for u in ups))
        for k in ("gx0", "ghl", "ghu"):
            worst = max(worst, _rel(_np(r[k][i]), ref[k]))
        for k in ("geps", "gf", "gw"):
            worst = max(worst, _rel(_np(r[k][:, i]), ref[k]))
        yi = ys[:, i]
        assert (_np(r["geps"][:, i])[yi == 0] == 0).all()
        for k in SHARED[:6]:
            total[k] = total.get(k, 0.0) + ref[k]
        total["glbz"] = total.get("glbz", 0.0) + ref["ghl"][q.m:]
        total["gubz"] = total.get("gubz", 0.0) + ref["ghu"][q.m:]
    for k in SHARED:
        if s[k] is None:
            assert (k in ("gG", "gE") and q.m == 0) or (k in ("glbz", "gubz") and not q.nbox), k
            continue
        worst = max(worst, _rel(_np(s[k]), total[k]))
    return worst


def _assert_error(what, worst, dt):
    print(f"{what} {'fp64' if dt == F64 else 'fp32'}: worst relative error {worst:.3e} "
          f"(tolerance {TOL[dt]:.3e})")
    assert TOL[F64] <= CEILING_F64 and TOL[F32] <= FINDING_F32
    assert worst <= TOL[dt], worst


def _acts(ref):
    """(b, T, mt) row states of a list of LoopQP.host_loop results."""
    return [r[2] for r in ref]


# ------------------------------------------------------------------ (a)
@DT
@pytest.mark.parametrize("nx,nu,N", lc.SHAPES)
def test_kernel_vs_recursion_shapes(dev, nx, nu, N, dt):
    """Every poly_loop_vjp_kernel<T, BS>, BS = 1..8: E = Phi, a state box and an
    input box, sets that change along the episode."""
    p = lc.shape_problem(nx, nu, N)
    assert (p["qp"].mt + 7) // 8 == lc.SHAPES.index((nx, nu, N)) + 1
    _assert_error(f"({nx},{nu},{N})", _case_error(p["qp"], p["x0"], lc.SHAPE_T, dev, dt,
                                                  sets=_acts(p["ref"])), dt)


@DT
@pytest.mark.parametrize("N", [5, 10])
def test_kernel_vs_recursion_session(dev, N, dt):
    """The session-2 MPC, the seven X0_SESSION, T = 12."""
    q, ref = lc.session_reference("Problem", N)
    _assert_error(f"session N={N}", _case_error(q, lc.X0_SESSION, lc.T_EPISODE, dev, dt,
                                                sets=_acts(ref)), dt)


@DT
def test_kernel_vs_recursion_drift(dev, dt):
    """The first 20 steps of the drift scenario: a disturbance w at every step."""
    q, w, ref = lc.drift_reference()
    T = 20
    _assert_error("drift", _case_error(q, np.zeros((2, 2)), T, dev, dt, w=w[:T],
                                       sets=_acts(ref)), dt)


@DT
def test_kernel_vs_recursion_config4(dev, dt):
    """n = 200 > 64 (four trips of the lane loops over z, the last partial),
    nx = 12, nu = 4, no box, E = None."""
    p = lc.config4_problem()
    _assert_error("config 4", _case_error(p["qp"], p["x0"], lc.SHAPE_T, dev, dt,
                                          sets=_acts(p["ref"])), dt)


def _affine_terms(q, T, batch):
    """Per-instance g (T, b, n) and e (T, b, m): a tenth of the scale of F x0 and
    a twentieth of the smallest finite row bound."""
    rng = np.random.default_rng(4242)
    g = 0.1 * rng.standard_normal((T, batch, q.n))
    width = np.abs(q.hu[np.isfinite(q.hu)]).min()
    e = 0.05 * width * rng.uniform(-1, 1, (T, batch, q.m))
    return g, e


@DT
def test_kernel_vs_recursion_affine(dev, dt):
    """mpcqp_mpc_poly_loop_affine with per-instance g and e.  The recursion
    takes (z_t, y_t) as given; that they are the step's optimum is checked here
    from the KKT conditions with g and e in place."""
    p = lc.shape_problem(*lc.SHAPES[1])
    q, x0, T = p["qp"], p["x0"], lc.SHAPE_T
    g, e = _affine_terms(q, T, x0.shape[0])
    if dt == F64:
        dq = _device_qp(q, dev)
        o, _ = _forward(q, dq, x0, T, dev, g=g, e=e)
        xs, zs, ys = _np(o["xs"]), _np(o["zs"]), _np(o["ys"])
        assert (ys != 0).any()
        for t in range(T):
            for i in range(x0.shape[0]):
                f = q.F @ xs[t, i] + g[t, i]
                assert np.abs(q.H @ zs[t, i] + f + q.Call.T @ ys[t, i]).max() < 1e-8 * (
                    1 + np.abs(f).max())
        assert lv.separation(q, xs[:, 0], zs[:, 0], ys[:, 0], e=e[:, 0]) > 0
    _assert_error("affine", _case_error(q, x0, T, dev, dt, g=_rounded(g, dt), e=_rounded(e, dt)),
                  dt)


# ------------------------------------------------------------------ (b)
def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


@DT
@pytest.mark.parametrize("which", ["shape", "config4"])
def test_one_step_is_poly_solve_vjp(dev, which, dt):
    """T = 1, gus = gxs = None, E = None: gf, geps, ghl, ghu are those of
    mpcqp_poly_solve_vjp(ys[0], gzs[0], gys[0]) bit for bit; gx0 (another order
    of the sums over the active rows and j) within the tolerance."""
    p = lc.shape_problem(*lc.SHAPES[5]) if which == "shape" else lc.config4_problem()
    q, x0 = p["qp"], p["x0"]
    dq = _device_qp(q, dev, dt)
    o, (A, B, E) = _forward(q, dq, x0, 1, dev, dt)
    assert (batched.status_code(o["status"]) == OPT).all() and (o["ys"] != 0).any()
    _, (gxs, gus, gzs, gys) = _upstream(q, 1, x0.shape[0], dev, dt)
    r = _raw(dq, A, B, None, o["ys"], o["status"], None, None, gzs, gys)
    one = poly_diff.poly_solve_vjp(dq, o["ys"][0], gzs[0], gys[0], status=o["status"][0])
    torch.cuda.synchronize()
    assert (r["vstatus"] == OPT).all() and (one["vstatus"] == OPT).all()
    for got, ref in ((r["gf"][0], one["gf"]), (r["geps"][0], one["e"]), (r["ghl"], one["ghl"]),
                     (r["ghu"], one["ghu"])):
        assert torch.equal(_bits(got), _bits(ref))
    assert r["gf"].abs().max() > 0 and r["geps"].abs().max() > 0
    assert (r["gw"] == 0).all()
    assert _rel(_np(r["gx0"]), _np(one["gx0"])) <= TOL[dt]


@DT
@pytest.mark.parametrize("shape", lc.SHAPES[:2], ids=["bs1", "bs2"])
def test_every_step_is_poly_solve_vjp(dev, shape, dt):
    """The loop reloads and re-sweeps W at every step: with B = 0 and gus = None
    v = 0 at every step, so geps[t] and gf[t] of a T = 3 episode are those of
    mpcqp_poly_solve_vjp(ys[t], gzs[t], gys[t]) bit for bit, at every t, on the
    instances both call OPTIMAL (all of them here).  The grids are the two
    smallest: m_total <= 8 (BS = 1) and 8 < m_total <= 16 (BS = 2)."""
    T, batch = 3, 4
    p = lc.shape_problem(*shape)
    q, x0 = p["qp"], p["x0"][:batch]
    assert (q.mt + 7) // 8 == lc.SHAPES.index(shape) + 1
    dq = _device_qp(q, dev, dt)
    o, (A, B, E) = _forward(q, dq, x0, T, dev, dt)
    assert (batched.status_code(o["status"]) == OPT).all() and (o["ys"] != 0).any()
    rng = np.random.default_rng(31)
    gzs = _t(rng.standard_normal((T, batch, q.n)), dev, dt)
    gys = _t(rng.standard_normal((T, batch, q.mt)), dev, dt)
    r = poly_diff.poly_loop_vjp(dq, A, torch.zeros_like(B), o["ys"], None, None, gzs, gys, E=E,
                                status=o["status"], need=("geps", "gf"))
    assert r["geps"].abs().max() > 0 and r["gf"].abs().max() > 0
    for t in range(T):
        one = poly_diff.poly_solve_vjp(dq, o["ys"][t], gzs[t], gys[t], status=o["status"][t])
        both = (r["vstatus"] == OPT) & (one["vstatus"] == OPT)
        assert both.all(), (t, r["vstatus"], one["vstatus"])
        for k, got, ref in (("geps", r["geps"][t], one["e"]), ("gf", r["gf"][t], one["gf"])):
            assert torch.equal(_bits(got[both]), _bits(ref[both])), (t, k)


# ------------------------------------------------------------------ (c)
def test_box_only_vs_box_loop_adjoint(dev):
    """m = 0: the same episode through mpcqp_mpc_box_loop (whose z holds active
    rows at the bound itself) and mpcqp_mpc_box_loop_vjp."""
    full, _ = lc.session_reference("Problem", 5)   # without its state box: both sides held
    q = lc.LoopQP(full.H, full.F, None, None, None, None, full.lbz, full.ubz, full.A, full.B)
    x0, T = lc.X0_SESSION, lc.T_EPISODE
    batch = x0.shape[0]
    dq = _device_qp(q, dev)
    o, (A, B, E) = _forward(q, dq, x0, T, dev)
    Hp, F, lb, ub = _t(pv.pack_lower(q.H), dev), _t(q.F, dev), _t(q.lbz, dev), _t(q.ubz, dev)
    ob = batched.mpc_box_loop(A, B, None, None, None, 5, _t(x0, dev), lb, ub, T, plans=True,
                              condensed={"H": Hp, "F": F})
    assert (batched.status_code(o["status"]) == OPT).all()
    assert (batched.status_code(ob["status"]) == OPT).all()
    held = (ob["zs"] == lb) | (ob["zs"] == ub)
    assert held.eq(o["ys"] != 0).all() and held.any() and (~held).any()
    _, (gxs, gus, gzs, gys) = _upstream(q, T, batch, dev, F64)
    r = _raw(dq, A, B, None, o["ys"], o["status"], gxs, gus, gzs, None)
    s = poly_diff.loop_shared_grads(dq, o["xs"], o["us"], o["zs"], o["ys"], r["gf"], r["geps"],
                                    r["gw"], r["vstatus"])
    rb = batched.mpc_box_loop_vjp(Hp, F, A, B, lb, ub, ob["xs"], ob["zs"], gxs, gus, gzs,
                                  status=ob["status"])
    assert (r["vstatus"] == OPT).all() and (rb["vstatus"] == OPT).all()
    pairs = [(r["gx0"], rb["gx0"]), (r["gf"], rb["gg"]), (r["gw"], rb["gw"]),
             (r["ghl"].sum(0), rb["glb"]), (r["ghu"].sum(0), rb["gub"]), (s["gH"], rb["gH"]),
             (s["gF"], rb["gF"]), (s["gA"], rb["gA"]), (s["gB"], rb["gB"]),
             (s["glbz"], rb["glb"]), (s["gubz"], rb["gub"])]
    worst = max(_rel(_np(a), _np(b).reshape(_np(a).shape)) for a, b in pairs)
    print(f"box only vs mpcqp_mpc_box_loop_vjp: worst relative difference {worst:.3e}")
    assert worst <= TOL[F64] + BOX_LOOP_VJP_TOL_F64, worst


# ------------------------------------------------------------ (d) NULL arguments
def _small(dev, dt=F64, T=lc.SHAPE_T):
    p = lc.shape_problem(*lc.SHAPES[1])
    q, x0 = p["qp"], p["x0"]
    dq = _device_qp(q, dev, dt)
    o, plant = _forward(q, dq, x0, T, dev, dt)
    assert (batched.status_code(o["status"]) == OPT).all() and (o["ys"] != 0).any()
    _, ups = _upstream(q, T, x0.shape[0], dev, dt)
    return q, dq, o, plant, ups


def test_null_outputs(dev):
    q, dq, o, (A, B, E), ups = _small(dev)
    full = _raw(dq, A, B, E, o["ys"], o["status"], *ups)
    for k in OUTS:
        assert torch.isfinite(full[k]).all() and full[k].abs().max() > 0
    for n_out in range(len(OUTS)):
        for outs in itertools.combinations(OUTS, n_out):
            r = _raw(dq, A, B, E, o["ys"], o["status"], *ups, outs=outs)
            assert set(r) == set(outs) | {"vstatus"} and (r["vstatus"] == OPT).all()
            for k in outs:
                assert torch.equal(r[k], full[k]), (outs, k)


def test_null_upstreams_status_and_e(dev):
    """A NULL upstream is a zero one; NULL status is all OPTIMAL; without gzs
    there is no scratch; NULL E is a zero E."""
    q, dq, o, (A, B, E), ups = _small(dev)
    ys, st = o["ys"], o["status"]
    for k in range(4):
        some = [u if j != k else None for j, u in enumerate(ups)]
        zero = [u if j != k else torch.zeros_like(u) for j, u in enumerate(ups)]
        a = _raw(dq, A, B, E, ys, st, *some, scratch=None if k == 2 else "alloc")
        b = _raw(dq, A, B, E, ys, st, *zero)
        for name in (*OUTS, "vstatus"):
            assert torch.equal(a[name], b[name]), (k, name)
    a = _raw(dq, A, B, E, ys, None, None, None, None, None, scratch=None)
    assert (a["vstatus"] == OPT).all()
    for name in OUTS:
        assert (a[name] == 0).all(), name
    a = _raw(dq, A, B, E, ys, None, *ups)
    b = _raw(dq, A, B, E, ys, st, *ups)
    for name in (*OUTS, "vstatus"):
        assert torch.equal(a[name], b[name]), name
    a = _raw(dq, A, B, None, ys, st, *ups)
    b = _raw(dq, A, B, torch.zeros_like(E), ys, st, *ups)
    for name in (*OUTS, "vstatus"):
        assert torch.equal(a[name], b[name]), name
    assert not torch.equal(a["gx0"], _raw(dq, A, B, E, ys, st, *ups)["gx0"])


def test_zero_steps(dev):
    q, dq, o, (A, B, E), ups = _small(dev)
    batch = o["ys"].shape[1]
    gxs = ups[0][:1].contiguous()
    empty = o["ys"][:0].contiguous()
    for args in ((empty, o["status"][:0].contiguous(), gxs), (None, None, gxs), (None, None, None)):
        r = _raw(dq, A, B, E, *args, steps=0, batch=batch, scratch=None)
        assert (r["vstatus"] == OPT).all()
        assert torch.equal(r["gx0"], gxs[0] if args[2] is not None else torch.zeros_like(gxs[0]))
        assert (r["ghl"] == 0).all() and (r["ghu"] == 0).all()
        assert r["geps"].numel() == 0 and r["gf"].numel() == 0 and r["gw"].numel() == 0


def test_small_scratch_and_wrapper_errors(dev):
    q, dq, o, (A, B, E), ups = _small(dev)
    ys, st = o["ys"], o["status"]
    T, batch = ys.shape[:2]
    need = poly_diff.loop_scratch_bytes(dq, batch, T)
    assert need > 0 and poly_diff.loop_scratch_bytes(dq, batch, 0) == 0
    small = torch.empty((need - 1,), dtype=torch.uint8, device=dev)
    with pytest.raises(nat.MpcqpError, match="mpcqp_mpc_poly_loop_vjp.*scratch"):
        _raw(dq, A, B, E, ys, st, *ups, scratch=small)
    _raw(dq, A, B, E, ys, st, ups[0], ups[1], None, ups[3], scratch=small)   # not needed without gzs
    with pytest.raises(ValueError, match="scratch"):
        poly_diff.poly_loop_vjp(dq, A, B, ys, gzs=ups[2], scratch=small)
    with pytest.raises(ValueError, match="unknown"):
        poly_diff.poly_loop_vjp(dq, A, B, ys, need=("gq",))
    with pytest.raises(ValueError, match="ys must be"):
        poly_diff.poly_loop_vjp(dq, A, B, ys[:, :, :-1])
    with pytest.raises(ValueError, match="gus must be"):
        poly_diff.poly_loop_vjp(dq, A, B, ys, gus=ups[1][:-1])
    with pytest.raises(ValueError, match="E must be"):
        poly_diff.poly_loop_vjp(dq, A, B, ys, E=E[:-1])
    with pytest.raises(ValueError, match="A must be"):
        poly_diff.poly_loop_vjp(dq, A[:1], B, ys)
    with pytest.raises(ValueError, match="status must be"):
        poly_diff.poly_loop_vjp(dq, A, B, ys, status=st[:-1])
    with pytest.raises(ValueError, match="gH needs gf"):
        poly_diff.loop_shared_grads(dq, o["xs"], o["us"], o["zs"], ys, None, None, None,
                                    torch.zeros(batch, dtype=torch.int32, device=dev), need=("gH",))
    r = poly_diff.poly_loop_vjp(dq, A, B, ys, *ups, E=E, status=st, need=("gx0", "gw"))
    assert r["gf"] is None and r["geps"] is None and r["gx0"] is not None
    raw = _raw(dq, A, B, E, ys, st, *ups)
    assert torch.equal(r["gx0"], raw["gx0"]) and torch.equal(r["gw"], raw["gw"])


# ------------------------------------------------------------ (e) status rules
def _spoiled(dq, A, B, E, ys, st, ups, bad, codes):
    """The instances ``bad`` get ``codes`` and exact zeros in every output, their
    per-step rows included; the others are OPTIMAL with the bits they have in a
    batch of their own."""
    o = _raw(dq, A, B, E, ys, st, *ups)
    batch = ys.shape[1]
    good = [i for i in range(batch) if i not in bad]
    sel = lambda t: None if t is None else t[:, good].contiguous()  # noqa: E731
    alone = _raw(dq, A, B, E, sel(ys), sel(st), *(sel(u) for u in ups))
    vs = o["vstatus"].tolist()
    assert [vs[i] for i in bad] == list(codes), vs
    assert [vs[i] for i in good] == [OPT] * len(good), vs
    assert (alone["vstatus"] == OPT).all()
    for k in ("gx0", "ghl", "ghu"):
        assert (o[k][bad] == 0).all(), k
        assert torch.equal(_bits(o[k][good]), _bits(alone[k])), k
    for k in ("geps", "gf", "gw"):
        assert (o[k][:, bad] == 0).all(), k
        assert torch.equal(_bits(o[k][:, good]), _bits(alone[k])), k
    for k in OUTS:
        assert torch.isfinite(alone[k]).all(), k
    for k in ("gx0", "gf", "gw"):
        assert alone[k].abs().max() > 0, k
    return o, good


def _session(dev, N=5, T=lc.T_EPISODE, **kw):
    q, _ = lc.session_reference("Problem", N)
    dq = _device_qp(q, dev)
    o, plant = _forward(q, dq, lc.X0_SESSION, T, dev, **kw)
    _, ups = _upstream(q, T, len(lc.X0_SESSION), dev, F64)
    return q, dq, o, plant, ups


def test_status_forward_infeasible(dev):
    """Problem(u_min = -2) loses feasibility at step 4 from (-60, 25); its
    neighbours in the batch do not.  The shared gradients are finite and those
    of the batch without the failed instance."""
    N, x_bad, t_bad = lc.INFEASIBLE_CASES[0]
    q = lc.infeasible_qp(N)
    x0 = np.array([lc.FEASIBLE_NEIGHBOUR, x_bad, (-90.0, 0.0)])
    T = t_bad + 3
    dq = _device_qp(q, dev)
    o, (A, B, E) = _forward(q, dq, x0, T, dev)
    code = batched.status_code(o["status"]).cpu().numpy()
    assert (code[:, [0, 2]] == OPT).all() and (code[:t_bad, 1] == OPT).all()
    assert code[t_bad, 1] == INFEAS and torch.isnan(o["ys"][t_bad, 1]).all()
    _, ups = _upstream(q, T, 3, dev, F64)
    r, good = _spoiled(dq, A, B, E, o["ys"], o["status"], ups, [1], [INFEAS])
    s = poly_diff.loop_shared_grads(dq, o["xs"], o["us"], o["zs"], o["ys"], r["gf"], r["geps"],
                                    r["gw"], r["vstatus"])
    sel = lambda t: t[:, good].contiguous()  # noqa: E731
    s2 = poly_diff.loop_shared_grads(dq, sel(o["xs"]), sel(o["us"]), sel(o["zs"]), sel(o["ys"]),
                                     sel(r["gf"]), sel(r["geps"]), sel(r["gw"]), r["vstatus"][good])
    for k in SHARED:
        assert torch.isfinite(s[k]).all(), k
        assert torch.allclose(s[k], s2[k], rtol=1e-12, atol=1e-12 * float(s2[k].abs().max())), k
    # without the forward's status the NaN in ys is found here
    assert _raw(dq, A, B, E, o["ys"], None, *ups)["vstatus"].tolist() == [OPT, NONFIN, OPT]


def test_status_forward_maxiter(dev):
    """max_iter = 3: the instances that need more at some step end MAXITER there."""
    q, dq, o, (A, B, E), ups = _session(dev, max_iter=3)
    code = batched.status_code(o["status"]).cpu().numpy()      # (T, b)
    bad = [i for i in range(code.shape[1]) if (code[:, i] != OPT).any()]
    first = [int(code[np.argmax(code[:, i] != OPT), i]) for i in bad]
    assert bad and len(bad) < code.shape[1] and MAXIT in first, code
    _spoiled(dq, A, B, E, o["ys"], o["status"], ups, bad, first)


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["gxs", "gus", "gzs", "gys"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_status_nonfinite_upstream(dev, which, value):
    q, dq, o, (A, B, E), ups = _session(dev)
    ups = [u.clone() for u in ups]
    ups[which][3, 2, -1] = value
    _spoiled(dq, A, B, E, o["ys"], o["status"], ups, [2], [NONFIN])


def test_status_softened_bit(dev):
    """A status word with MPCQP_STATUS_SOFTENED: the step solved a softened
    problem; the instance is INFEASIBLE for the adjoint of the hard loop."""
    q, dq, o, (A, B, E), ups = _session(dev)
    st = o["status"].clone()
    st[5, 4] |= nat.STATUS_SOFTENED
    _spoiled(dq, A, B, E, o["ys"], st, ups, [4], [INFEAS])


def test_status_indefinite_h(dev):
    """The setup's flag: every instance NOT_CONVEX, through the forward's status
    and, without it, through the flag itself."""
    p = lc.shape_problem(*lc.SHAPES[1])
    q, x0, T = p["qp"], p["x0"], 3
    H = q.H.copy()
    H[1, 1] = -1.0
    bad = lc.LoopQP(H, q.F, q.G, q.E, q.hl, q.hu, q.lbz, q.ubz, q.A, q.B)
    dq = _device_qp(bad, dev)
    o, (A, B, E) = _forward(bad, dq, x0, T, dev)
    assert (batched.status_code(o["status"]) == NOTCVX).all()
    _, ups = _upstream(q, T, x0.shape[0], dev, F64)
    for status, ys in ((o["status"], o["ys"]), (None, torch.zeros_like(o["ys"]))):
        r = _raw(dq, A, B, E, ys, status, *ups)
        assert (r["vstatus"] == NOTCVX).all()
        for k in OUTS:
            assert (r[k] == 0).all(), k


def test_status_dependent_active_rows(dev):
    """The row of v_1 in Gam moves with u_0 alone: marked active together with
    the box row of u_0 it makes M_AA singular, found at the second pivot of that
    step; the rows of the later steps, written before, are zeroed too."""
    q, dq, o, (A, B, E), ups = _session(dev)
    assert q.G[1, 0] != 0 and not q.G[1, 1:].any()
    ys = o["ys"].clone()
    ys[2, 3] = 0.0
    ys[2, 3, 1] = ys[2, 3, q.m] = 1.0
    _spoiled(dq, A, B, E, ys, o["status"], ups, [3], [NOTCVX])


# ------------------------------------------------------------------ (f) autograd
GC = dict(eps=1e-6, atol=1e-6, rtol=1e-5)   # those of tests/test_gpu_poly_vjp.py
NB, TG = 3, 3                               # instances and steps of a gradcheck


def _leaf(a, dev):
    return _t(a, dev).requires_grad_(True)


def _small_plant(nx, nu, seed):
    rng = np.random.default_rng(seed)
    A = 0.5 * np.eye(nx) + 0.2 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
    return A, 0.5 * rng.standard_normal((nx, nu))


def _gradcheck_args(dev, which):
    """Leaves H, G, F, A, B, x0, hl, hu, lbz, ubz, E, w, g, e of a small loop."""
    rng = np.random.default_rng(31)
    if which == "3x2":
        c = pv.family_a(3, 2)
        n, m, nx, nu = c.n, c.m, c.nx, 1
        A, B = _small_plant(nx, nu, 5)
        H, G, F, x0, hl, hu, lbz, ubz = c.H, c.G, c.F, c.x0[:NB], c.hl[:NB], c.hu[:NB], c.lbz, c.ubz
        E = 0.1 * rng.standard_normal((m, nx))
    else:
        p = lc.shape_problem(*lc.SHAPES[1])
        q = p["qp"]
        n, m, nx, nu = q.n, q.m, q.nx, q.nu
        H, G, F, A, B, E, x0 = q.H, q.G, q.F, q.A, q.B, q.E, p["x0"][[0, 3, 4]]  # 0, 3: state rows held
        hl, hu, lbz, ubz = q.hl, q.hu, q.lbz, q.ubz
    w = 0.05 * rng.standard_normal((TG, NB, nx))
    g = 0.05 * rng.standard_normal((TG, NB, n))
    e = 0.01 * rng.standard_normal((TG, m))
    return tuple(_leaf(a, dev) for a in (pv.pack_lower(H), G, F, A, B, x0, hl, hu, lbz, ubz, E, w,
                                         g, e))


def _loop_fn(*a):
    return ag.poly_loop_diff(*a[:10], steps=TG, E=a[10], w=a[11], g=a[12], e=a[13])[:4]


@pytest.mark.parametrize("which", ["3x2", "shape"])
def test_gradcheck_poly_loop_diff(dev, which):
    """A loss on xs, us, zs and ys; per-instance x0, w, g (and hl, hu at 3x2),
    shared e, lbz, ubz, H (packed), G, F, E and the plant A, B."""
    args = _gradcheck_args(dev, which)
    xs, us, zs, ys, st = ag.poly_loop_diff(*args[:10], steps=TG, E=args[10], w=args[11],
                                           g=args[12], e=args[13])
    assert (batched.status_code(st) == OPT).all() and (ys != 0).any()
    assert all(t.requires_grad for t in (xs, us, zs, ys)) and not st.requires_grad
    assert torch.autograd.gradcheck(_loop_fn, args, **GC)


def test_values_are_those_of_polyqp_loop(dev):
    args = _gradcheck_args(dev, "shape")
    H, G, F, A, B, x0, hl, hu, lbz, ubz, E, w, g, e = (a.detach() for a in args)
    dq = batched.PolyQP(H, G, F, lbz, ubz)
    ref = dq.loop(A, B, x0, TG, hl, hu, E, w, plans=True, multipliers=True, g=g, e=e)
    for got in (_loop_fn(*args), _loop_fn(*(a.detach() for a in args)),
                ag.poly_loop_diff(*args[:10], steps=TG, E=args[10], w=args[11], g=args[12],
                                  e=args[13], qp=dq)[:4]):
        for a, k in zip(got, ("xs", "us", "zs", "ys")):
            assert torch.equal(_bits(a.detach()), _bits(ref[k])), k
    st = ag.poly_loop_diff(*args[:10], steps=TG, E=args[10], w=args[11], g=args[12], e=args[13])[4]
    assert torch.equal(st, ref["status"])
    # a loss on xs and us alone: the backward runs without gzs and gys
    xs, us = _loop_fn(*args)[:2]
    grads = torch.autograd.grad(xs.sum() + (us * us).sum(), args, allow_unused=True)
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)


X0_MPC = np.array([(-50.0, 20.0), (-40.0, 25.0), (-20.0, 22.0)])  # those of test_gpu_poly_vjp.py
T_MPC = 4
# For the difference quotients of the tracking episode (x_ref = (-10, 0)): the
# forward's round-off in y is about 2.2e-16 * cond(M_AA) * max|y|, and a quotient
# with eps = 1e-6 divides it by 1e-6.  At (-50, 20) the oracle has cond * max|y|
# = 4.3e4 (quotients of 2e-6, above atol, were seen there for entries whose
# derivative is zero: rounding alone); at these three it is 3.3e3, 4.0e2 and
# 1.2e2, with the velocity row held at the first and box rows at all three,
# separated by > 0.2.
X0_TRACK = np.array([(-38.0, 24.8), (-33.0, 23.5), (-12.0, 10.0)])


def test_gradcheck_mpc_poly_loop_diff(dev):
    """Session-2 Problem at N = 5, T = 4: x0, xlo, xhi, lb, ub, Q, R, Qf, w and
    a state reference.  Weights enter as full matrices and are symmetrised
    inside, as in tests/test_gpu_poly_vjp.py."""
    p = Problem()
    N = 5
    A, B = _t(p.A, dev), _t(p.B, dev)
    rng = np.random.default_rng(77)
    w = 0.1 * rng.standard_normal((T_MPC, len(X0_TRACK), 2))
    x_ref = np.array([-10.0, 0.0])
    args = tuple(_leaf(np.asarray(a, float), dev) for a in (
        X0_TRACK, p.x_min, p.x_max, p.u_min, p.u_max, p.Q, p.R, p.Q, w, x_ref))
    sym = lambda W: 0.5 * (W + W.transpose(-1, -2))  # noqa: E731

    def fn(x0, xlo, xhi, lb, ub, Q, R, Qf, w, x_ref):
        return ag.mpc_poly_loop_diff(A, B, sym(Q), sym(R), sym(Qf), N, x0, xlo, xhi, lb, ub,
                                     steps=T_MPC, w=w, x_ref=x_ref)[:4]

    plain = [a.detach() for a in args]
    xs, us, zs, ys, st = ag.mpc_poly_loop_diff(A, B, *plain[5:8], N, *plain[:5], steps=T_MPC,
                                               w=plain[8], x_ref=plain[9])
    assert (batched.status_code(st) == OPT).all() and not xs.requires_grad
    assert (ys[:, :, :2 * N] != 0).any() and (ys[:, :, 2 * N:] != 0).any()
    o = batched.mpc_poly_loop(A, B, *plain[5:8], N, *plain[:5], steps=T_MPC, w=plain[8],
                              x_ref=plain[9], plans=True, multipliers=True)
    for a, k in zip((xs, us, zs, ys, st), ("xs", "us", "zs", "ys", "status")):
        assert torch.equal(a, o[k]), k
    assert torch.autograd.gradcheck(fn, args, **GC)


def test_plant_gets_gradients(dev):
    """plant = (A_p, B_p): the simulated plant's gradients are the recursion's
    sums of gw_t x_t' and gw_t u_t'."""
    p = Problem()
    A, B, Q, R = (_t(a, dev) for a in (p.A, p.B, p.Q, p.R))
    Ap, Bp = _leaf(p.A * 0.99, dev), _leaf(p.B * 1.05, dev)

    def fn(Ap, Bp):
        return ag.mpc_poly_loop_diff(A, B, Q, R, Q, 5, _t(X0_MPC, dev), p.x_min, p.x_max, p.u_min,
                                     p.u_max, steps=T_MPC, plant=(Ap, Bp))[:4]

    assert (batched.status_code(ag.mpc_poly_loop_diff(
        A, B, Q, R, Q, 5, _t(X0_MPC, dev), p.x_min, p.x_max, p.u_min, p.u_max, steps=T_MPC,
        plant=(Ap, Bp))[4]) == OPT).all()
    assert torch.autograd.gradcheck(fn, (Ap, Bp), **GC)


def test_autograd_errors(dev):
    p = Problem()
    A, B, Q, R = (_t(a, dev) for a in (p.A, p.B, p.Q, p.R))
    x0 = _t(X0_MPC, dev)
    with pytest.raises(NotImplementedError, match="A and B"):
        ag.mpc_poly_loop_diff(A.clone().requires_grad_(True), B, Q, R, Q, 5, x0, -150.0, 25.0,
                              steps=2)
    with pytest.raises(NotImplementedError, match="A and B"):
        ag.mpc_poly_loop_diff(A, B.clone().requires_grad_(True), Q, R, Q, 5, x0, -150.0, 25.0,
                              steps=2)
    with pytest.raises(ValueError, match="shared by the batch"):
        ag.mpc_poly_loop_diff(A[None], B, Q, R, Q, 5, x0, -150.0, 25.0, steps=2)
    with pytest.raises(ValueError, match="xlo"):
        ag.mpc_poly_loop_diff(A, B, Q, R, Q, 5, x0, _t(np.zeros(3), dev), 25.0, steps=2)
    # nx = 5 is outside the limits of the adjoint of condensing
    eye5 = torch.eye(5, dtype=F64, device=dev)
    A5, B5 = eye5 * 0.9, torch.ones((5, 1), dtype=F64, device=dev)
    x5 = torch.ones((2, 5), dtype=F64, device=dev)
    with pytest.raises(NotImplementedError, match="nx <= 4"):
        ag.mpc_poly_loop_diff(A5, B5, eye5.clone().requires_grad_(True), R, eye5, 3, x5, -9.0, 9.0,
                              steps=2)
    xs = ag.mpc_poly_loop_diff(A5, B5, eye5, R, eye5, 3, x5.clone().requires_grad_(True), -9.0, 9.0,
                               steps=2)[0]
    assert xs.requires_grad
    args = _gradcheck_args(dev, "3x2")
    with pytest.raises(TypeError, match="soft"):
        ag.poly_loop_diff(*args[:10], steps=2, soft=(1.0, 1.0))
    import model_predictive_control_amd as pkg
    assert pkg.poly_loop_diff is ag.poly_loop_diff
    assert pkg.mpc_poly_loop_diff is ag.mpc_poly_loop_diff


# ------------------------------------------------------------------ (g)
def test_graph_capture_forward_backward(dev):
    """Forward and backward captured in one graph, the adjoint called with a
    preallocated scratch and through autograd: two replays give the same bits,
    those of the eager run."""
    p = lc.shape_problem(*lc.SHAPES[3])
    q, x0, T = p["qp"], p["x0"], lc.SHAPE_T
    dq = _device_qp(q, dev)
    batch = x0.shape[0]
    _, ups = _upstream(q, T, batch, dev, F64)
    scratch = torch.empty((poly_diff.loop_scratch_bytes(dq, batch, T),), dtype=torch.uint8,
                          device=dev)
    fixed = [_t(a, dev) for a in (pv.pack_lower(q.H), q.G, q.F, q.A, q.B)]
    tail = [_t(a, dev) for a in (q.lbz, q.ubz)]

    def leaves():
        return [_leaf(a, dev) for a in (x0, q.hl, q.hu, q.E)]

    def run(x0_, hl, hu, E):
        A, B = fixed[3], fixed[4]
        o = dq.loop(A, B, x0_.detach(), T, hl.detach(), hu.detach(), E.detach(), plans=True,
                    multipliers=True)
        r = poly_diff.poly_loop_vjp(dq, A, B, o["ys"], *ups, E=E.detach(), status=o["status"],
                                    scratch=scratch)
        xs, us, zs, ys, _ = ag.poly_loop_diff(*fixed, x0_, hl, hu, *tail, steps=T, E=E, qp=dq)
        loss = sum((a * u).sum() for a, u in zip((xs, us, zs, ys), ups))
        gr = torch.autograd.grad(loss, (x0_, hl, hu, E))
        return [t.detach() for t in (xs, zs, ys, r["gx0"], r["ghl"], r["ghu"], r["gf"], r["geps"],
                                     r["gw"], *gr)]

    eager = [t.clone() for t in run(*leaves())]
    assert torch.equal(eager[3], eager[9])
    static = leaves()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(*static)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(out, eager):
            assert torch.equal(_bits(a), _bits(e))
