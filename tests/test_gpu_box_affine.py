"""GPU parity: mpcqp_mpc_box_loop_affine -- the receding-horizon loop of
tests/test_gpu_loop_box.py with a per-step linear term g_t in the gradient and
a plant disturbance w_t -- against oracle.qp.box_qp on the same QP
(tests/_box_affine_cases.py), always at the device's own recorded state xs[t].
What tests/test_box_affine_host.py certifies about the scenarios on the
reference alone is listed there."""
import numpy as np
import pytest
import torch

import _box_affine_cases as bc
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import batched
from model_predictive_control_amd.closed_loop import lti_box_mpc_loop

pytestmark = pytest.mark.gpu

OPT, MAXIT, NOTCVX, INFEAS, NONFIN = 0, 1, 2, 3, 4
KEYS = ("xs", "us", "zs", "status")


def _t(a, dev, dt=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _np(r):
    torch.cuda.synchronize()
    return {k: (v.double().cpu().numpy() if v.is_floating_point() else v.cpu().numpy())
            for k, v in r.items() if isinstance(v, torch.Tensor)}


def _loop_t(p, dev, *, g=None, w=None, cold=False, steps=bc.T, dt=torch.float64, lb=None, ub=None,
            **kw):
    """batched.mpc_box_loop on the scenario p (per-instance plants and bounds),
    tensors out."""
    return batched.mpc_box_loop(_t(p["A"], dev, dt), _t(p["B"], dev, dt), _t(p["Q"], dev, dt),
                                _t(p["R"], dev, dt), _t(p["Qf"], dev, dt), p["N"],
                                _t(p["x0"], dev, dt), _t(p["lb"] if lb is None else lb, dev, dt),
                                _t(p["ub"] if ub is None else ub, dev, dt), steps, plans=True,
                                g=_t(g, dev, dt), w=_t(w, dev, dt), cold=cold, **kw)


def _loop(*a, **kw):
    return _np(_loop_t(*a, **kw))


def _entry(p, dev, steps, *, g=None, w=None, flags=0):
    """mpcqp_mpc_box_loop_affine called directly (g, w tensors or None):
    (rc, outputs)."""
    b, nx, nu = p["x0"].shape[0], p["B"].shape[1], p["B"].shape[2]
    N, n = p["N"], p["N"] * p["B"].shape[2]
    A, Bm, x0, lb, ub = (_t(p[k], dev) for k in ("A", "B", "x0", "lb", "ub"))
    cd = batched.condense(A, Bm, _t(p["Q"], dev), _t(p["R"], dev), _t(p["Qf"], dev), N,
                          outputs=("H", "F"))
    f64 = dict(dtype=torch.float64, device=dev)
    o = dict(xs=torch.zeros((steps + 1, b, nx), **f64), us=torch.zeros((max(steps, 1), b, nu), **f64),
             zs=torch.zeros((max(steps, 1), b, n), **f64),
             status=torch.zeros((max(steps, 1), b), dtype=torch.int32, device=dev))
    ptr = batched._ptr
    rc = nat.load().mpcqp_mpc_box_loop_affine(
        nat.F64, b, nx, nu, N, steps, flags, ptr(cd["H"]), n * (n + 1) // 2, ptr(cd["F"]), n * nx,
        ptr(A), nx * nx, ptr(Bm), nx * nu, ptr(x0), nx, ptr(lb), n, ptr(ub), n, ptr(g),
        0 if g is None or g.ndim == 2 else n, ptr(w), ptr(o["xs"]), ptr(o["us"]), ptr(o["zs"]),
        ptr(o["status"]), 0, 0.0, batched._stream())
    torch.cuda.synchronize()
    return rc, o


def _code(r):
    return r["status"] & 0xFF


def _same(a, b, keys=KEYS, sel=None):
    """torch.equal on every output (of the instances sel), NaNs in the same
    places counting as equal."""
    for k in keys:
        x, y = a[k], b[k]
        if sel is not None:
            x, y = x[:, sel], y[:, sel]
        if x.is_floating_point():
            assert torch.equal(x.isnan(), y.isnan()), k
            x, y = x.nan_to_num(), y.nan_to_num()
        assert torch.equal(x, y), k


def _check(p, r, g=None, w=None, fp32=False, plant=None):
    A, Bm, cds = plant or (p["A"], p["B"], p["cd"])
    return max(bc.check_episode(A[i], Bm[i], cds[i]["H"], cds[i]["F"], p["lb"], p["ub"], r["xs"],
                                r["us"], r["zs"], i, g, w, fp32=fp32) for i in range(bc.B))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("what", ["g", "w", "gw"])
@pytest.mark.parametrize("nx,nu,N", bc.SHAPES)
def test_every_step_against_oracle(dev, nx, nu, N, what):
    """Every step at the device's own state: the plan is the oracle's argmin
    with f = F xs[t] + g_t, the applied input its first move, the next state
    A xs[t] + B us[t] + w_t; all OPTIMAL."""
    p = bc.problem(nx, nu, N)
    g = p["g"] if "g" in what else None
    w = p["w"] if "w" in what else None
    r = _loop(p, dev, g=g, w=w)
    assert (_code(r) == OPT).all(), _code(r)
    assert np.array_equal(r["xs"][0], p["x0"])
    worst = _check(p, r, g, w)
    print(f"({nx}, {nu}, {N}) {what}: worst relative z error {worst:.2e}")
    if what == "gw":        # the same states as the oracle's own loop while both are exact
        for i in range(bc.B):
            xs = p["ref"][i][0]
            assert np.abs(r["xs"][:, i] - xs).max() < 1e-7 * (1 + np.abs(xs).max()), i


# ------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("nx,nu,N", [(2, 1, 8), (3, 2, 16)])
def test_null_and_zero_arguments(dev, nx, nu, N):
    """g = w = NULL, flags = 0 through the new entry point is
    mpcqp_mpc_box_loop bit for bit; all-zero g and w give equal values and
    status words."""
    p = bc.problem(nx, nu, N)
    plain = _loop_t(p, dev)
    torch.cuda.synchronize()
    assert (_code(plain) == OPT).all()
    rc, o = _entry(p, dev, bc.T)
    assert rc == 0, nat.load().mpcqp_last_error()
    for k in KEYS:
        assert torch.equal(o[k], plain[k]), k
    pn = _np(plain)
    n = N * nu
    for shape in ((bc.T, n), (bc.T, bc.B, n)):
        z = _loop(p, dev, g=np.zeros(shape), w=np.zeros((bc.T, bc.B, nx)))
        for k in KEYS:
            assert np.array_equal(z[k], pn[k]), (k, shape)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("nx,nu,N", [(2, 1, 8), (4, 1, 32)])
def test_shared_against_broadcast(dev, nx, nu, N):
    """g (T, n) with strideG = 0 against the same values broadcast to (T, b, n)."""
    p = bc.problem(nx, nu, N)
    g = p["g"][:, 0]
    gb = np.repeat(g[:, None], bc.B, axis=1)
    rs, rb = _loop_t(p, dev, g=g, w=p["w"]), _loop_t(p, dev, g=gb, w=p["w"])
    torch.cuda.synchronize()
    assert (_code(rs) == OPT).all()
    _same(rs, rb)
    _check(p, _np(rs), g, p["w"])


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("nx,nu,N", [(2, 1, 8), (2, 2, 11)])
def test_cold_start(dev, nx, nu, N):
    """MPCQP_LOOP_COLD changes the path, not the answer; every cold step sweeps
    all n rows before it iterates."""
    p = bc.problem(nx, nu, N)
    warm = _loop(p, dev, g=p["g"], w=p["w"])
    cold = _loop(p, dev, g=p["g"], w=p["w"], cold=True)
    assert (_code(warm) == OPT).all() and (_code(cold) == OPT).all()
    scale = np.maximum(1.0, np.abs(warm["zs"]).max(axis=-1, keepdims=True))
    assert (np.abs(cold["zs"] - warm["zs"]) < 1e-9 * scale).all()
    _check(p, cold, p["g"], p["w"])
    its = (cold["status"] >> 8) & 0xFFFF
    assert (its >= N * nu).all(), its
    # cold without g or w is still the same loop
    plain = _loop(p, dev)
    c0 = _loop(p, dev, cold=True)
    assert (_code(c0) == OPT).all()
    assert (np.abs(c0["zs"] - plain["zs"]) < 1e-9 * np.maximum(1.0, np.abs(plain["zs"]).max())).all()
    assert (((c0["status"] >> 8) & 0xFFFF) >= N * nu).all()


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("nx,nu,N", [(2, 1, 8), (3, 2, 16)])
def test_equals_per_step_path(dev, nx, nu, N):
    """One batched.solve_box over the T * b QPs with f = F x_t + g_t at the
    loop's recorded states gives its plans."""
    p = bc.problem(nx, nu, N)
    n, b, T = N * nu, bc.B, bc.T
    r = _loop_t(p, dev, g=p["g"], w=p["w"])
    A, Bm = _t(p["A"], dev), _t(p["B"], dev)
    cd = batched.condense(A, Bm, _t(p["Q"], dev), _t(p["R"], dev), _t(p["Qf"], dev), N,
                          outputs=("H", "F"))
    f = torch.einsum("bij,tbj->tbi", cd["F"], r["xs"][:T]) + _t(p["g"], dev)
    H = cd["H"][None].expand(T, b, -1).reshape(T * b, -1)
    lb = _t(p["lb"], dev)[None].expand(T, b, n).reshape(T * b, n)
    ub = _t(p["ub"], dev)[None].expand(T, b, n).reshape(T * b, n)
    z, st = batched.solve_box(H, f.reshape(T * b, n), lb, ub)
    torch.cuda.synchronize()
    assert (batched.status_code(st) == 0).all() and (_code(r) == OPT).all()
    z = z.reshape(T, b, n)
    scale = z.abs().amax(dim=-1, keepdim=True).clamp(min=1.0)
    assert ((r["zs"] - z).abs() < 1e-9 * scale).all()


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("nx,nu,N,j", [(2, 1, 8, 3), (3, 2, 16, 21)])
def test_nan_in_g(dev, nx, nu, N, j):
    """NaN in g[2, i0, j] (j = 21: the lane's second row): NONFINITE from step 2
    on for i0 only, NaN outputs there; every other instance, those of i0's
    wavefront included, equals the clean run bitwise."""
    p = bc.problem(nx, nu, N)
    t0, i0 = 2, 1
    clean = _loop_t(p, dev, g=p["g"], w=p["w"])
    g2 = p["g"].copy()
    g2[t0, i0, j] = np.nan
    r = _loop_t(p, dev, g=g2, w=p["w"])
    torch.cuda.synchronize()
    code = _code(r).cpu().numpy()
    assert (code[:t0, i0] == OPT).all() and (code[t0:, i0] == NONFIN).all(), code
    for k in ("us", "zs"):
        assert r[k][t0:, i0].isnan().all(), k
        assert torch.equal(r[k][:t0, i0], clean[k][:t0, i0]), k
    assert torch.equal(r["xs"][:t0 + 1, i0], clean["xs"][:t0 + 1, i0])
    assert r["xs"][t0 + 1:, i0].isnan().all()
    _same(r, clean, sel=[i for i in range(bc.B) if i != i0])


# ------------------------------------------------------------------ 8
def test_inf_in_w(dev):
    """Inf in w[2, i0]: step 2 is solved (finite input), x_3 is not finite and
    steps >= 3 report NONFINITE through the state test."""
    p = bc.problem(2, 1, 8)
    t0, i0 = 2, 3
    clean = _loop_t(p, dev, g=p["g"], w=p["w"])
    w2 = p["w"].copy()
    w2[t0, i0, 1] = np.inf
    r = _loop_t(p, dev, g=p["g"], w=w2)
    torch.cuda.synchronize()
    code = _code(r).cpu().numpy()
    assert (code[:t0 + 1, i0] == OPT).all() and (code[t0 + 1:, i0] == NONFIN).all(), code
    assert r["us"][t0, i0].isfinite().all() and r["zs"][t0, i0].isfinite().all()
    assert torch.equal(r["zs"][:t0 + 1, i0], clean["zs"][:t0 + 1, i0])
    assert not r["xs"][t0 + 1, i0].isfinite().all()
    assert r["us"][t0 + 1:, i0].isnan().all() and r["zs"][t0 + 1:, i0].isnan().all()
    assert r["xs"][t0 + 2:, i0].isnan().all()
    _same(r, clean, sel=[i for i in range(bc.B) if i != i0])


# ------------------------------------------------------------------ 9
def test_status_precedence(dev):
    """lb > ub together with a NaN in g[0]: NONFINITE, not INFEASIBLE; lb > ub
    alone stays INFEASIBLE; the rest is the oracle's."""
    p = bc.problem(2, 1, 8)
    i0, i1 = 2, 4
    lb, ub = p["lb"].copy(), p["ub"].copy()
    lb[i0, 3], ub[i0, 3] = 1.0, -1.0
    lb[i1, 0], ub[i1, 0] = 1.0, -1.0
    g2 = p["g"].copy()
    g2[0, i0, 5] = np.nan
    r = _loop(p, dev, g=g2, w=p["w"], lb=lb, ub=ub)
    code = _code(r)
    assert (code[:, i0] == NONFIN).all() and (code[:, i1] == INFEAS).all(), code
    assert (code[:, [0, 1, 3]] == OPT).all(), code
    assert np.isnan(r["zs"][:, [i0, i1]]).all() and np.isnan(r["xs"][1:, [i0, i1]]).all()
    for i in (0, 1, 3):
        bc.check_episode(p["A"][i], p["B"][i], p["cd"][i]["H"], p["cd"][i]["F"], p["lb"], p["ub"],
                         r["xs"], r["us"], r["zs"], i, g2, p["w"])


# ------------------------------------------------------------------ 10, 11
def test_small_step_counts_and_bad_flags(dev):
    """steps = 0 records x0 only; steps = 1 reads exactly one row of g and w (the
    prefetch of a step that does not exist is not issued); an unknown flag bit
    is MPCQP_EINVAL."""
    p = bc.problem(2, 1, 8)
    g1, w1 = _t(p["g"][:1], dev), _t(p["w"][:1], dev)
    assert tuple(g1.shape) == (1, bc.B, 8)
    rc, o = _entry(p, dev, 0, g=g1, w=w1)
    assert rc == 0, nat.load().mpcqp_last_error()
    assert np.array_equal(o["xs"][0].cpu().numpy(), p["x0"])
    assert (o["status"] == 0).all() and (o["us"] == 0).all()      # untouched
    rc, o = _entry(p, dev, 1, g=g1, w=w1)
    assert rc == 0, nat.load().mpcqp_last_error()
    r = _np(o)
    assert (_code(r) == OPT).all()
    _check(p, r, p["g"][:1], p["w"][:1])
    for flags in (1, 8, nat.LOOP_COLD | 4):
        rc, _ = _entry(p, dev, 1, g=g1, w=w1, flags=flags)
        assert rc == -1 and b"flags" in nat.load().mpcqp_last_error(), flags
    with pytest.raises(ValueError):
        _loop_t(p, dev, g=p["g"][:, :4])
    with pytest.raises(ValueError):
        _loop_t(p, dev, w=p["w"][:-1])
    with pytest.raises(ValueError):
        _loop_t(p, dev, g=p["g"], x_ref=torch.zeros(2, dtype=torch.float64, device=dev))


# ------------------------------------------------------------------ 12
@pytest.mark.parametrize("nx,nu,N", bc.FP32_SHAPES)
def test_fp32(dev, nx, nu, N):
    """fp32 episodes against the fp64 oracle on the fp32-rounded plant, g and w,
    at the device's states, with the fp32 tolerance of the box loop."""
    p = bc.problem(nx, nu, N)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    g32, w32 = f32(p["g"]), f32(p["w"])
    r = _loop(p, dev, g=g32, w=w32, dt=torch.float32)
    assert (_code(r) == OPT).all(), _code(r)
    A32, B32 = f32(p["A"]), f32(p["B"])
    cds = [bc.oc.condense(A32[i], B32[i], p["Q"], p["R"], p["Qf"], N) for i in range(bc.B)]
    worst = _check(p, r, g32, w32, fp32=True, plant=(A32, B32, cds))
    print(f"fp32 ({nx}, {nu}, {N}): worst relative z error {worst:.3e}")


# ------------------------------------------------------------------ 13
def test_tracking_end_to_end(dev):
    """The FHC double integrator to the setpoint (p*, 0) under |u| <= 1:
    mpc_box_loop(x_ref=) is the oracle's loop, equals mpc_poly_loop(x_ref=) with
    no state box (another kernel on the same problem), and lti_box_mpc_loop
    reaches the setpoint as closely as the oracle does."""
    sp = bc.setpoint()
    T, N, b = bc.SP_T, bc.SP_N, 3
    t = lambda a: _t(a, dev)  # noqa: E731
    x0 = np.zeros((b, 2))
    xr = np.array([bc.SP_PSTAR, 0.0])
    r = batched.mpc_box_loop(t(sp["A"]), t(sp["B"]), t(sp["Q"]), t(sp["R"]), t(sp["Qf"]), N, t(x0),
                             -1.0, 1.0, T, plans=True, x_ref=t(xr), u_ref=t(np.zeros(1)))
    rn = _np(r)
    assert (_code(rn) == OPT).all(), _code(rn)
    assert (np.abs(rn["us"][:3]) == 1.0).all()                   # saturated at first
    for i in range(b):
        assert (np.abs(rn["xs"][:, i] - sp["xs"]) < 1e-9 * (1 + np.abs(sp["xs"]))).all(), i
        bc.check_episode(sp["A"], sp["B"], sp["cd"]["H"], sp["cd"]["F"], -1.0, 1.0, rn["xs"],
                         rn["us"], rn["zs"], i, sp["g"])
    q = _np(batched.mpc_poly_loop(t(sp["A"]), t(sp["B"]), t(sp["Q"]), t(sp["R"]), t(sp["Qf"]), N,
                                  t(x0), None, None, -1.0, 1.0, T, plans=True, x_ref=t(xr),
                                  u_ref=t(np.zeros(1))))
    assert (_code(q) == OPT).all(), _code(q)
    assert np.abs(q["xs"] - rn["xs"]).max() < 1e-8 and np.abs(q["zs"] - rn["zs"]).max() < 1e-8
    out = lti_box_mpc_loop(sp["A"], sp["B"], sp["Q"], sp["R"], sp["Qf"], N, x0, -1.0, 1.0, T,
                           x_ref=sp["x_ref"])
    torch.cuda.synchronize()
    assert out["success"].all()
    te = out["tracking_error"].cpu().numpy()
    assert te.shape == (T, b, 2)
    assert np.array_equal(te, out["xs"].cpu().numpy()[1:] - sp["x_ref"][1:T + 1][:, None, :])
    last = np.abs(te[-1]).max()
    print(f"tracking error at the last step {last:.3e} (oracle {bc.SP_ORACLE_LAST:.1e})")
    assert last < bc.SP_LAST_BOUND


# ------------------------------------------------------------------ 14
def test_tracking_terms_per_instance_plants(dev):
    """tracking_terms with a per-instance Gam (b, N*nx, n) against the NumPy
    formula per instance; the shapes accepted before against the same formula;
    and mpc_box_loop(x_ref=, u_ref=) on per-instance plants against the oracle."""
    nx, nu, N = 3, 2, 16
    p = bc.problem(nx, nu, N)
    T, b, n = bc.T, bc.B, N * nu
    rng = np.random.default_rng(14)
    x_ref = rng.normal(size=(T + N + 1, nx))
    u_ref = 0.1 * rng.normal(size=(b, T + N, nu))
    Gam = np.stack([d["Gam"] for d in p["cd"]])
    Q, R, Qf = p["Q"], p["R"], p["Qf"]
    want = np.stack([bc.tracking_g(Gam[i], Q, R, Qf, N, T, x_ref, u_ref[i]) for i in range(b)], 1)
    tq = (_t(Q, dev), _t(R, dev), _t(Qf, dev))
    got = batched.tracking_terms({"Gam": _t(Gam, dev)}, *tq, N, T, _t(x_ref, dev), _t(u_ref, dev))
    assert tuple(got.shape) == (T, b, n)
    assert np.abs(got.cpu().numpy() - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    got = batched.tracking_terms({"Gam": _t(Gam, dev)}, *tq, N, T, _t(x_ref, dev))
    want_x = np.stack([bc.tracking_g(Gam[i], Q, R, Qf, N, T, x_ref) for i in range(b)], 1)
    assert np.abs(got.cpu().numpy() - want_x).max() < 1e-12 * max(1.0, np.abs(want_x).max())
    # shared Gam: the shapes accepted before, unchanged
    g0 = batched.tracking_terms({"Gam": _t(Gam[0], dev)}, *tq, N, T, _t(x_ref, dev))
    assert tuple(g0.shape) == (T, n)
    assert np.abs(g0.cpu().numpy() - want_x[:, 0]).max() < 1e-12 * max(1.0, np.abs(want_x).max())
    gb = batched.tracking_terms({"Gam": _t(Gam[0], dev)}, *tq, N, T, _t(x_ref, dev),
                                _t(u_ref, dev))
    want_b = np.stack([bc.tracking_g(Gam[0], Q, R, Qf, N, T, x_ref, u_ref[i]) for i in range(b)], 1)
    assert tuple(gb.shape) == (T, b, n)
    assert np.abs(gb.cpu().numpy() - want_b).max() < 1e-12 * max(1.0, np.abs(want_b).max())
    with pytest.raises(ValueError):
        batched.tracking_terms({"Gam": _t(Gam[:3], dev)}, *tq, N, T, _t(x_ref, dev), _t(u_ref, dev))
    # end to end on per-instance plants
    r = _loop(p, dev, x_ref=_t(x_ref, dev), u_ref=_t(u_ref, dev))
    assert (_code(r) == OPT).all(), _code(r)
    _check(p, r, want)


# ------------------------------------------------------------------ 15
def test_graph_capture(dev):
    """The entry point only enqueues: captured in a graph and replayed twice it
    gives the eager result."""
    p = bc.problem(2, 1, 8)
    eager = _loop_t(p, dev, g=p["g"], w=p["w"])
    torch.cuda.synchronize()
    args = [_t(p[k], dev) for k in ("A", "B", "Q", "R", "Qf")]
    x0, lb, ub, g, w = (_t(p[k], dev) for k in ("x0", "lb", "ub", "g", "w"))
    cd = batched.condense(*args, p["N"], outputs=("H", "F"))
    out = {k: torch.zeros_like(eager[k]) for k in KEYS}

    def run():
        batched.mpc_box_loop(*args, p["N"], x0, lb, ub, bc.T, plans=True, condensed=cd, out=out,
                             g=g, w=w)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        for k in KEYS:
            out[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(eager, out)
