"""GPU: the box-QP adjoint kernel (mpcqp_solve_box_vjp) against the NumPy
closed form of tests/_box_vjp_cases.py, its status rules, and the autograd
functions built on it (solve_box_diff, mpc_box_diff).

Errors are max|device - reference| / (1 + max|reference|) per output array.
Tolerances: ten times the largest such error measured over every case of
test_kernel_vs_closed_form (printed by the test itself):
  fp64  measured 7.803e-13 (at n = 32, cond(H) = 4.4e4; 1.5e-13 at the config-2
        shape n = 20), so the tolerance 7.803e-12 is well under the ceiling
        1e-9 = n cond(H) eps (~1.3e-11 at config 2) with two decades of margin;
  fp32  measured 5.194e-5 (n = 32) against the fp64 closed form on fp32-rounded
        data and the device's own fp32 z: tolerance 5.194e-4.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _box_vjp_cases as vc
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import autograd as ag
from model_predictive_control_amd import batched

pytestmark = pytest.mark.gpu

MEASURED_F64 = 7.803e-13
MEASURED_F32 = 5.194e-5
TOL_F64 = 10 * MEASURED_F64
TOL_F32 = 10 * MEASURED_F32
CEILING_F64 = 1e-9
OUTS = ("gf", "glb", "gub", "gH", "vstatus")
INF = float("inf")


def _cases(n):
    """Eight session-1 instances with mixed active sets (x0 ~ U(-3, 3)^2)."""
    return vc.session1_batch(n, 8, 11, 3.0)


def _t(a, dev, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / (1 + np.abs(ref).max()))


def _raw(H, z, lb, ub, gz, status=None, outs=OUTS):
    """mpcqp_solve_box_vjp as it is: per-instance outputs, only those in
    ``outs`` passed (the rest NULL), pre-filled with NaN / -1 so that an entry
    the kernel leaves out shows.  H, lb, ub: 1-D means shared (stride 0)."""
    batch, n = z.shape
    P = n * (n + 1) // 2
    o = {k: torch.full((batch, P if k == "gH" else n), float("nan"), dtype=z.dtype,
                       device=z.device) for k in outs if k != "vstatus"}
    if "vstatus" in outs:
        o["vstatus"] = torch.full((batch,), -1, dtype=torch.int32, device=z.device)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = lambda t, w: 0 if t is None or t.ndim == 1 else w  # noqa: E731
    rc = nat.load().mpcqp_solve_box_vjp(
        nat.F64 if z.dtype == torch.float64 else nat.F32, batch, n, p(H), s(H, P), p(z), p(lb),
        s(lb, n), p(ub), s(ub, n), p(status), p(gz), p(o.get("gf")), p(o.get("glb")),
        p(o.get("gub")), p(o.get("gH")), p(o.get("vstatus")), torch.cuda.current_stream().cuda_stream)
    nat.check(rc, "mpcqp_solve_box_vjp")
    torch.cuda.synchronize()
    return o


def _reference(H, z, lb, ub, g):
    """Closed form per instance on float64 copies of what the device saw."""
    b, n = z.shape
    lb = np.full((b, n), -INF) if lb is None else np.broadcast_to(lb, (b, n))
    ub = np.full((b, n), INF) if ub is None else np.broadcast_to(ub, (b, n))
    Hb = np.broadcast_to(H, (b, n, n))
    cf = [vc.closed_form(Hb[i], z[i], lb[i], ub[i], g[i]) for i in range(b)]
    return {k: np.stack([c[s] for c in cf]) for k, s in
            (("gf", "d"), ("glb", "glb"), ("gub", "gub"), ("gH", "gH"))}


def _bounds(kind, b, n):
    lb, ub = -np.ones((b, n)), np.ones((b, n))
    if kind == "no_lb":
        lb = None
    elif kind == "no_ub":
        ub = None
    elif kind == "inf_rows":
        lb[:, 0] = -INF
        ub[:, n - 1] = INF
    return lb, ub


def _kernel_case(dev, dt, n, batch, kind, shared):
    """Forward on the device, adjoint on the device's z, closed form on the
    same (dtype-rounded) data.  Returns the worst error over gf, glb, gub, gH."""
    p = _cases(n)
    npdt = np.float64 if dt == torch.float64 else np.float32
    rnd = lambda a: None if a is None else np.asarray(a, npdt).astype(np.float64)  # noqa: E731
    scale = np.ones(batch) if shared else 1 + 0.25 * np.arange(batch)
    H = rnd(p["H"][0]) if shared else rnd(p["H"][:batch] * scale[:, None, None])
    f, g = rnd(p["f"][:batch]), rnd(p["g"][:batch])
    lb, ub = _bounds(kind, batch, n)
    Hd = _t(vc.pack_lower(H), dev, dt)
    opt = lambda a: None if a is None else _t(a, dev, dt)  # noqa: E731
    z, st = batched.solve_box(Hd, _t(f, dev, dt), opt(lb), opt(ub))
    assert (batched.status_code(st) == 0).all(), st
    o = _raw(Hd, z, opt(lb), opt(ub), _t(g, dev, dt), st)
    assert (o["vstatus"] == 0).all()
    zn = z.cpu().numpy().astype(np.float64)
    ref = _reference(H, zn, lb, ub, g)
    on = (zn == (-INF if lb is None else lb)) | (zn == (INF if ub is None else ub))
    return max(_rel(o[k].cpu().numpy().astype(np.float64), ref[k]) for k in ref), on


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 4, 5, 17, 20, 29, 32])
def test_kernel_vs_closed_form(dev, n, dt):
    """Every BS edge, idle groups and a partly filled wavefront, per-instance
    and shared H, bounds given / NULL / +-inf on single rows."""
    worst, act, free = 0.0, False, False
    for batch, kind, shared in itertools.product((1, 3, 5, 8), ("both", "no_lb", "no_ub", "inf_rows"),
                                                 (False, True)):
        err, on = _kernel_case(dev, dt, n, batch, kind, shared)
        worst = max(worst, err)
        act |= bool(on.any())
        free |= bool((~on).any())
    print(f"n={n} {dt}: worst relative error {worst:.3e}")
    assert act and (free or n == 1)
    if dt == torch.float64:
        assert TOL_F64 <= CEILING_F64
    assert worst <= (TOL_F64 if dt == torch.float64 else TOL_F32), worst


def test_null_output_combinations(dev):
    """Each subset of the outputs passed alone gives what the full call gives."""
    n, batch = 20, 5
    p = _cases(n)
    Hd = _t(vc.pack_lower(p["H"][:batch]), dev)
    lb, ub = _t(p["lb"][:batch], dev), _t(p["ub"][:batch], dev)
    z, st = batched.solve_box(Hd, _t(p["f"][:batch], dev), lb, ub)
    g = _t(p["g"][:batch], dev)
    full = _raw(Hd, z, lb, ub, g, st)
    for r in range(len(OUTS)):
        for outs in itertools.combinations(OUTS, r):
            o = _raw(Hd, z, lb, ub, g, st, outs=outs)
            assert set(o) == set(outs)
            for k in outs:
                assert torch.equal(o[k], full[k]), (outs, k)


def _mixed_instances(n, dev):
    """z, lb, ub, g, status rows of: an all-free instance, an all-active one, a
    half-active one, and one the forward gave up on (no sweeps, zeros)."""
    rng = np.random.default_rng(40 + n)
    z = rng.uniform(-0.5, 0.5, (4, n))
    lb, ub = np.full((4, n), -INF), np.full((4, n), INF)
    lb[1] = z[1]                       # all at lb
    ub[1, ::3] = z[1, ::3]             # ... some of them at both
    lb[2, ::2] = z[2, ::2]             # half active: even rows at lb,
    ub[2, 1::4] = z[2, 1::4]           # some odd rows at ub
    lb[3, :2] = z[3, :2]
    status = np.array([0, 0, 0, nat.STATUS_MAXITER | (7 << 8)], dtype=np.int32)
    g = rng.standard_normal((4, n))
    return (_t(z, dev), _t(lb, dev), _t(ub, dev), _t(g, dev),
            torch.as_tensor(status, device=dev))


@pytest.mark.parametrize("n", [20, 32])
def test_mixed_wavefront_permutations(dev, n):
    """One wave, four different free sets: every instance's result is bitwise
    what it is alone in a batch of one, wherever it sits -- also next to a slot
    past the end of the batch."""
    p = _cases(n)
    Hd = _t(vc.pack_lower(p["H"][:4] * (1 + 0.25 * np.arange(4))[:, None, None]), dev)
    z, lb, ub, g, st = _mixed_instances(n, dev)
    alone = [_raw(Hd[i:i + 1], z[i:i + 1], lb[i:i + 1], ub[i:i + 1], g[i:i + 1], st[i:i + 1])
             for i in range(4)]
    H0 = p["H"][0] * 1.0
    ref = _reference(np.stack([H0 * (1 + 0.25 * i) for i in range(4)]), z.cpu().numpy(),
                     lb.cpu().numpy(), ub.cpu().numpy(), g.cpu().numpy())
    # the instances are what they are meant to be
    assert (alone[0]["glb"] == 0).all() and (alone[0]["gub"] == 0).all()
    assert _rel(alone[0]["gf"].cpu().numpy(), ref["gf"][:1]) <= TOL_F64
    assert (alone[1]["gf"] == 0).all() and (alone[1]["gH"] == 0).all()
    assert torch.equal(alone[1]["glb"], g[1:2])
    assert _rel(alone[2]["gf"].cpu().numpy(), ref["gf"][2:3]) <= TOL_F64
    assert _rel(alone[2]["glb"].cpu().numpy(), ref["glb"][2:3]) <= TOL_F64
    assert _rel(alone[2]["gub"].cpu().numpy(), ref["gub"][2:3]) <= TOL_F64
    assert int(alone[3]["vstatus"][0]) == nat.STATUS_MAXITER
    assert all((alone[3][k] == 0).all() for k in ("gf", "glb", "gub", "gH"))
    perms = list(itertools.permutations(range(4))) + list(itertools.permutations(range(3)))
    for perm in perms:
        ix = torch.as_tensor(perm, device=dev)
        o = _raw(Hd[ix].contiguous(), z[ix].contiguous(), lb[ix].contiguous(), ub[ix].contiguous(),
                 g[ix].contiguous(), st[ix].contiguous())
        for pos, i in enumerate(perm):
            for k in OUTS:
                assert torch.equal(o[k][pos], alone[i][k][0]), (perm, pos, k)


def _status_problem(dev, n=20):
    p = _cases(n)
    ix = [0, 5, 2, 3]  # slot 1: the instance with the most active rows (and free ones)
    on = (p["z"][5] == p["lb"][5]) | (p["z"][5] == p["ub"][5])
    assert on.sum() >= 3 and (~on).any()
    return (_t(vc.pack_lower(p["H"][ix]), dev), _t(p["f"][ix], dev), _t(p["lb"][ix], dev),
            _t(p["ub"][ix], dev), _t(p["g"][ix], dev))


def _check_bad_instance(o, good, code):
    keep = [0, 2, 3]
    assert int(o["vstatus"][1]) == code
    assert o["vstatus"][keep].tolist() == [0, 0, 0]
    for k in ("gf", "glb", "gub", "gH"):
        assert (o[k][1] == 0).all(), k       # exact zeros, no NaN
        assert torch.equal(o[k][keep], good[k]), k


@pytest.mark.parametrize("bad", ["maxiter", "infeasible", "nonfinite", "nan_gz"])
def test_status_rules_bad_instance(dev, bad):
    """Instance 1 of 4 fails: zero gradients and the code in vstatus[1], the
    other three as in the run without it."""
    H, f, lb, ub, g = _status_problem(dev)
    keep = torch.as_tensor([0, 2, 3], device=dev)
    code = {"maxiter": nat.STATUS_MAXITER, "infeasible": nat.STATUS_INFEASIBLE,
            "nonfinite": nat.STATUS_NONFINITE, "nan_gz": nat.STATUS_NONFINITE}[bad]
    if bad == "infeasible":
        lb = lb.clone()
        lb[1, 3] = 2.0
    if bad == "nonfinite":
        f = f.clone()
        f[1, 2] = float("nan")
    z, st = batched.solve_box(H, f, lb, ub)
    if bad == "maxiter":
        z, st = batched.solve_box(H, f, lb, ub, max_iter=1)
        z0, st0 = batched.solve_box(H, f, lb, ub)
        assert int(batched.status_code(st)[1]) == nat.STATUS_MAXITER
        z = torch.where(torch.arange(4, device=dev)[:, None] == 1, z, z0)
        st = torch.where(torch.arange(4, device=dev) == 1, st, st0)
    if bad == "nan_gz":
        g = g.clone()
        g[1, 5] = float("nan")
    else:
        assert int(batched.status_code(st)[1]) == code
    assert batched.status_code(st)[keep].tolist() == [0, 0, 0]
    o = _raw(H, z, lb, ub, g, st)
    good = _raw(H[keep].contiguous(), z[keep].contiguous(), lb[keep].contiguous(),
                ub[keep].contiguous(), g[keep].contiguous(), st[keep].contiguous())
    _check_bad_instance(o, good, code)


def test_status_indefinite_free_block(dev):
    """H_FF indefinite (no forward status given): NOT_CONVEX and zeros; a
    non-finite H: NONFINITE and zeros; the neighbours untouched."""
    H, f, lb, ub, g = _status_problem(dev)
    z, st = batched.solve_box(H, f, lb, ub)
    keep = torch.as_tensor([0, 2, 3], device=dev)
    good = _raw(H[keep].contiguous(), z[keep].contiguous(), lb[keep].contiguous(),
                ub[keep].contiguous(), g[keep].contiguous())
    n = z.shape[1]
    free = int(torch.nonzero((z[1] != lb[1]) & (z[1] != ub[1]))[0])
    Hbad = H.clone()
    Hbad[1, free * (free + 1) // 2 + free] = -1.0
    _check_bad_instance(_raw(Hbad, z, lb, ub, g), good, nat.STATUS_NOT_CONVEX)
    Hbad[1, n] = float("inf")
    _check_bad_instance(_raw(Hbad, z, lb, ub, g), good, nat.STATUS_NONFINITE)


def test_batched_wrapper_sums_shared_inputs(dev):
    """batched.solve_box_vjp: shared H, lb, ub get the batch sum."""
    n, batch = 17, 5
    p = _cases(n)
    Hs = _t(vc.pack_lower(p["H"][0]), dev)
    lb, ub = _t(p["lb"][0], dev), _t(p["ub"][0], dev)
    z, st = batched.solve_box(Hs, _t(p["f"][:batch], dev), lb, ub)
    g = _t(p["g"][:batch], dev)
    raw = _raw(Hs, z, lb, ub, g, st)
    r = batched.solve_box_vjp(Hs, z, lb, ub, g, status=st)
    assert r["gH"].shape == Hs.shape and r["glb"].shape == lb.shape
    assert torch.equal(r["gf"], raw["gf"]) and torch.equal(r["vstatus"], raw["vstatus"])
    for k in ("gH", "glb", "gub"):
        assert torch.equal(r[k], raw[k].sum(0)), k
    assert batched.solve_box_vjp(Hs, z, lb, ub, g, need_H=False)["gH"] is None
    with pytest.raises(ValueError):
        batched.solve_box_vjp(Hs[:-1], z, lb, ub, g)
    with pytest.raises(ValueError):
        batched.solve_box_vjp(Hs, z, lb, ub, g[:, :-1])


# ------------------------------------------------------------------ autograd
GC = dict(eps=1e-6, atol=1e-6, rtol=1e-5)


def _mixed_nondegenerate(p, count):
    """``count`` non-degenerate instances, those with both active and free
    rows first (the margin is the oracle's)."""
    on = (p["z"] == p["lb"]) | (p["z"] == p["ub"])
    mixed = on.any(1) & ~on.all(1)
    idx = np.concatenate([np.nonzero(p["nondeg"] & mixed)[0], np.nonzero(p["nondeg"] & ~mixed)[0]])
    assert idx.size >= count
    assert mixed[idx[0]]
    return idx[:count]


def test_gradcheck_solve_box_per_instance(dev):
    p = vc.session1_batch(4)
    ix = _mixed_nondegenerate(p, 3)
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    args = (leaf(vc.pack_lower(p["H"][ix])), leaf(p["f"][ix]), leaf(p["lb"][ix]), leaf(p["ub"][ix]))
    assert torch.autograd.gradcheck(lambda H, f, lb, ub: ag.solve_box_diff(H, f, lb, ub)[0], args, **GC)


def test_gradcheck_solve_box_shared(dev):
    p = vc.random_batch(nx=3, nu=2, N=3)
    ix = _mixed_nondegenerate(p, 3)
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    args = (leaf(vc.pack_lower(p["H"][0])), leaf(p["f"][ix]), leaf(p["lb"][0]), leaf(p["ub"][0]))
    assert args[0].ndim == 1 and args[0].shape[0] == 21
    assert torch.autograd.gradcheck(lambda H, f, lb, ub: ag.solve_box_diff(H, f, lb, ub)[0], args, **GC)


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_instance"])
@pytest.mark.parametrize("shape", [(2, 1, 5), (4, 2, 3)], ids=["nx2nu1N5", "nx4nu2N3"])
def test_gradcheck_mpc_box(dev, shape, shared):
    """Weights enter as full matrices W and are symmetrised inside, so the
    numerical derivative moves Q_ij and Q_ji together and is compared with the
    symmetrised analytic gradient."""
    nx, nu, N = shape
    p = vc.session1_batch(5) if shape == (2, 1, 5) else vc.random_batch(nx=nx, nu=nu, N=N)
    ix = _mixed_nondegenerate(p, 3)
    rep = (lambda a: a) if shared else (lambda a: np.broadcast_to(a, (3,) + a.shape))
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    A, B = _t(p["A"], dev), _t(p["B"], dev)
    args = (leaf(rep(p["Q"])), leaf(rep(p["R"])), leaf(rep(p["Qf"])), leaf(p["x0"][ix]),
            leaf(p["lb"][ix]), leaf(p["ub"][ix]))
    sym = lambda W: 0.5 * (W + W.transpose(-1, -2))  # noqa: E731

    def fn(Q, R, Qf, x0, lb, ub):
        return ag.mpc_box_diff(A, B, sym(Q), sym(R), sym(Qf), N, x0, lb, ub)[0]

    z, st = ag.mpc_box_diff(A, B, *[a.detach() for a in args[:3]], N, *[a.detach() for a in args[3:]])
    assert (batched.status_code(st) == 0).all()
    assert np.abs(z.cpu().numpy() - p["z"][ix]).max() < 1e-9
    assert torch.autograd.gradcheck(fn, args, **GC)


def test_fixtures_against_oracle_active_set(dev, golden):
    """Device gradients from the device's z equal the closed form on the
    ORACLE's z on the 64 config-2 fixtures (same active set off degeneracy)."""
    gd = golden("boxqp_cfg2.npz")
    b, n = gd["z"].shape
    lb, ub = -np.ones((b, n)), np.ones((b, n))
    m = np.array([vc.margin(gd["H"][i], gd["f"][i], lb[i], ub[i], gd["z"][i]) for i in range(b)])
    use = m > vc.MARGIN
    assert b == 64 and (~use).sum() <= 2
    g = np.random.default_rng(64).standard_normal((b, n))
    Hd = _t(vc.pack_lower(gd["H"]), dev)
    z, st = batched.solve_box(Hd, _t(gd["f"], dev), -1.0, 1.0)
    o = _raw(Hd, z, _t(lb, dev), _t(ub, dev), _t(g, dev), st)
    ref = _reference(gd["H"], gd["z"], lb, ub, g)
    assert (o["vstatus"] == 0).all()
    worst = max(_rel(o[k].cpu().numpy()[use], ref[k][use]) for k in ref)
    print(f"fixtures: worst relative error {worst:.3e}, skipped {(~use).sum()}")
    assert worst <= TOL_F64, worst


def test_config2_batch_fills_grads(dev, golden):
    gd = golden("boxqp_cfg2.npz")
    b, n = gd["z"].shape
    leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
    H, f = leaf(vc.pack_lower(gd["H"])), leaf(gd["f"])
    lb, ub = leaf(-np.ones((b, n))), leaf(np.ones(n))
    z, st = ag.solve_box_diff(H, f, lb, ub)
    assert not st.requires_grad and z.requires_grad
    z.sum().backward()
    for t in (H, f, lb, ub):
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all()
    assert f.grad.abs().max() > 0 and lb.grad.abs().max() > 0 and ub.grad.abs().max() > 0
    # scalar bounds get no gradient, and nothing else changes
    H2, f2 = leaf(vc.pack_lower(gd["H"])), leaf(gd["f"])
    z2, _ = ag.solve_box_diff(H2, f2, -1.0, 1.0)
    z2.sum().backward()
    assert torch.equal(z2, z) and torch.equal(f2.grad, f.grad) and torch.equal(H2.grad, H.grad)


def test_mpc_box_diff_failed_instance_gives_zeros(dev):
    """Instance 1 of 4 has a NaN in x0: its forward ends NONFINITE, its
    condensed xbar and f are NaN, and still every gradient is finite -- its
    own entries exact zeros, the shared weights' sums what the other three
    instances give alone."""
    p = vc.session1_batch(5)
    ix = _mixed_nondegenerate(p, 4)
    A, B = _t(p["A"], dev), _t(p["B"], dev)
    w = _t(p["g"][ix], dev)

    def grads(x0, lbv, wv):
        leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
        Q, R, Qf, lb = leaf(p["Q"]), leaf(p["R"]), leaf(p["Qf"]), leaf(lbv)
        x0 = x0.clone().requires_grad_(True)
        z, st = ag.mpc_box_diff(A, B, Q, R, Qf, 5, x0, lb, 1.0)
        z.backward(wv)                      # dL/dz = w for every instance, the failed one too
        return st, dict(Q=Q.grad, R=R.grad, Qf=Qf.grad, x0=x0.grad, lb=lb.grad)

    x0 = _t(p["x0"][ix], dev)
    x0[1, 0] = float("nan")
    st, bad = grads(x0, p["lb"][ix], w)
    assert batched.status_code(st).tolist() == [0, nat.STATUS_NONFINITE, 0, 0]
    keep = [0, 2, 3]
    _, good = grads(x0[keep], p["lb"][ix][keep], w[keep])
    for k, g in bad.items():
        assert torch.isfinite(g).all(), k
    assert (bad["x0"][1] == 0).all() and (bad["lb"][1] == 0).all()
    assert torch.equal(bad["x0"][keep], good["x0"]) and torch.equal(bad["lb"][keep], good["lb"])
    for k in ("Q", "R", "Qf"):
        assert good[k].abs().max() > 0
        # the batch sum runs over 4 instead of 3 terms (one of them 0): same
        # terms, the summation order may differ
        assert torch.allclose(bad[k], good[k], rtol=1e-13, atol=0), k


def test_graph_capture_forward_backward(dev):
    """Forward and backward captured in one graph replay to the eager result.
    The eager reference runs on leaves of its own, and the captured leaves
    meet autograd first on the warm-up side stream, with no autograd graph kept
    from there: a gradient accumulator remembers the stream it was created on,
    and one made on the default stream would pull that stream into the capture."""
    n, batch = 20, 6
    p = _cases(n)
    w = _t(p["g"][:batch], dev)

    def leaves():
        leaf = lambda a: _t(a, dev).requires_grad_(True)  # noqa: E731
        return (leaf(vc.pack_lower(p["H"][:batch])), leaf(p["f"][:batch]), leaf(p["lb"][0]),
                leaf(p["ub"][:batch]))

    def run(H, f, lb, ub):
        z, _ = ag.solve_box_diff(H, f, lb, ub)
        return [t.detach() for t in (z,) + torch.autograd.grad((z * w).sum(), (H, f, lb, ub))]

    eager = [t.clone() for t in run(*leaves())]
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
            assert torch.equal(a, e)


def test_errors(dev):
    n = 40
    H = torch.eye(n, dtype=torch.float64, device=dev)
    Hp = batched.pack_lower(H)[None].repeat(2, 1)
    f = torch.ones((2, n), dtype=torch.float64, device=dev)
    z, st = ag.solve_box_diff(Hp, f, -1.0, 1.0)          # no gradient asked: the plain solve
    assert (batched.status_code(st) == 0).all() and not z.requires_grad
    with pytest.raises(NotImplementedError, match="32"):
        ag.solve_box_diff(Hp, f.clone().requires_grad_(True), -1.0, 1.0)
    p = vc.session1_batch(5)
    A, B = _t(p["A"], dev), _t(p["B"], dev)
    Q, R, Qf, x0 = _t(p["Q"], dev), _t(p["R"], dev), _t(p["Qf"], dev), _t(p["x0"][:3], dev)
    with pytest.raises(NotImplementedError, match="A, B"):
        ag.mpc_box_diff(A.clone().requires_grad_(True), B, Q, R, Qf, 5, x0, -1.0, 1.0)
    with pytest.raises(NotImplementedError):
        ag.mpc_box_diff(A, B.clone().requires_grad_(True), Q, R, Qf, 5, x0, -1.0, 1.0)
    with pytest.raises(NotImplementedError, match="32"):
        ag.mpc_box_diff(A, B, Q, R, Qf, 33, x0.clone().requires_grad_(True), -1.0, 1.0)
    import model_predictive_control_amd as pkg
    assert pkg.solve_box_diff is ag.solve_box_diff and pkg.mpc_box_diff is ag.mpc_box_diff
