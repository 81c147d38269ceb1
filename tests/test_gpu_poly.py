"""GPU parity: mpcqp_solve_poly vs the Goldfarb-Idnani oracle and the committed
session-2/3 golden minimisers (state box on x_1..x_N + input box, the OCP of
session_4/main.py:58-69 restricted to the linear session-2/3 plants)."""
import numpy as np
import pytest
import torch

import _poly_cases as pc
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import batched, problems
from oracle import condense as oc
from oracle import qp as oq

pytestmark = pytest.mark.gpu


def _t(a, dev, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


@pytest.mark.parametrize("tag,cls", [("session_2", problems.Problem), ("session_3", problems.Problem3)])
def test_poly_session_golden(dev, golden, tag, cls):
    gp = golden("polyqp_s2.npz")
    p = cls()
    N = p.N
    X0 = gp[f"{tag}_x0"]
    b = X0.shape[0]
    d = batched.condense(_t(p.A, dev), _t(p.B, dev), _t(p.Q, dev), _t(p.R, dev), _t(p.Q, dev), N,
                         x0=_t(X0, dev), outputs=("H", "f", "Gam", "xbar"))
    G = d["Gam"][0]
    hl = _t(np.tile(p.x_min, N), dev) - d["xbar"]
    hu = _t(np.tile(p.x_max, N), dev) - d["xbar"]
    z, y, st = batched.solve_poly(d["H"][0], d["f"], G, hl, hu, lbz=p.u_min, ubz=p.u_max)
    code = batched.status_code(st).cpu().numpy()
    z = z.cpu().numpy()
    feas = gp[f"{tag}_feasible"]
    assert (code[feas] == 0).all(), code
    assert (code[~feas] == 3).all(), code
    assert np.abs(z[feas] - gp[f"{tag}_z"][feas]).max() < 1e-8


@pytest.mark.parametrize("n,m", [(5, 3), (20, 20), (40, 24), (64, 40), (200, 40)])
def test_poly_random_polytope(dev, n, m):
    """Config-4 shape family: shared H, G (m rows, h > 0 so z = 0 is feasible)."""
    rng = np.random.default_rng(n * 131 + m)
    M = rng.normal(size=(n, n))
    H = M @ M.T / n + 0.5 * np.eye(n)
    G = rng.normal(size=(m, n))
    batch = 16 if n < 200 else 6
    f = rng.normal(size=(batch, n)) * 4
    h = rng.uniform(0.2, 1.0, size=(batch, m))
    z, y, st = batched.solve_poly(_t(oc.pack_lower(H), dev), _t(f, dev), _t(G, dev), None, _t(h, dev))
    z = z.cpu().numpy()
    y = y.cpu().numpy()
    assert (batched.status_code(st) == 0).all()
    for b in range(batch):
        zr, lam, _ = oq.poly_qp(H, f[b], G, h[b])
        assert np.abs(z[b] - zr).max() < 1e-8 * max(1, np.abs(zr).max()), np.abs(z[b] - zr).max()
        assert np.abs(np.maximum(y[b], 0) - lam).max() < 1e-6 * max(1, np.abs(lam).max())
        assert (G @ z[b] - h[b]).max() < 1e-9


def test_poly_two_sided_with_box(dev):
    rng = np.random.default_rng(3)
    n, m, batch = 12, 10, 20
    M = rng.normal(size=(n, n)); H = M @ M.T + np.eye(n)
    G = rng.normal(size=(m, n))
    f = rng.normal(size=(batch, n)) * 5
    hl = -rng.uniform(0.5, 1.0, (batch, m)); hu = rng.uniform(0.5, 1.0, (batch, m))
    z, y, st = batched.solve_poly(_t(oc.pack_lower(H), dev), _t(f, dev), _t(G, dev), _t(hl, dev),
                                  _t(hu, dev), lbz=-0.7, ubz=0.7)
    z = z.cpu().numpy()
    assert (batched.status_code(st) == 0).all()
    for b in range(batch):
        Gs = np.vstack([G, -G])
        hs = np.concatenate([hu[b], -hl[b]])
        zr, _, _ = oq.poly_qp(H, f[b], Gs, hs, lb=np.full(n, -0.7), ub=np.full(n, 0.7))
        assert np.abs(z[b] - zr).max() < 1e-8


@pytest.mark.parametrize("nx,nu,N,m,box", [(12, 4, 50, 40, False), (4, 2, 10, 12, True), (2, 1, 20, 6, True)])
def test_poly_parametric_x0(dev, nx, nu, N, m, box):
    """PolyQP: shared factors once (poly_setup), per-instance x0 -> z with the
    fused s0 / z epilogue; BASELINE config-4 shape first.  Checked against the
    Goldfarb-Idnani oracle on the explicitly condensed QP."""
    rng = np.random.default_rng(nx * 100 + N)
    U, _ = np.linalg.qr(rng.normal(size=(nx, nx)))
    A = (U * rng.uniform(0.5, 0.98, nx)) @ U.T
    B = rng.normal(size=(nx, nu)) / np.sqrt(nx)
    Q, R = np.eye(nx), 0.1 * np.eye(nu)
    n = N * nu
    d = oc.condense(A, B, Q, R, Q, N)
    G = rng.normal(size=(m, n))
    h = rng.uniform(0.5, 1.5, size=m)
    b = 24
    X0 = rng.normal(size=(b, nx)) * 3
    f1 = rng.normal(size=(b, n)) * 0.1
    lbz, ubz = (-0.4, 0.4) if box else (None, None)
    qp = batched.PolyQP(_t(oc.pack_lower(d["H"]), dev), _t(G, dev), _t(d["F"], dev), lbz, ubz)
    z, y, st = qp.solve(_t(X0, dev), _t(f1, dev), hu=_t(h, dev))
    assert (batched.status_code(st) == 0).all(), batched.status_code(st)
    z = z.cpu().numpy()
    for i in range(b):
        fi = d["F"] @ X0[i] + f1[i]
        zr = oq.poly_qp(d["H"], fi, G, h, None if lbz is None else np.full(n, lbz),
                        None if ubz is None else np.full(n, ubz))[0]
        assert np.abs(z[i] - zr).max() < 1e-8 * max(1.0, np.abs(zr).max()), np.abs(z[i] - zr).max()
    # same factors, gradient-only form (x0 = None) gives the same answer
    z2, _, st2 = qp.solve(None, _t(X0 @ d["F"].T + f1, dev), hu=_t(h, dev))
    assert (batched.status_code(st2) == 0).all()
    assert np.abs(z2.cpu().numpy() - z).max() < 1e-9


# ===================================================================== cases
# dual_range_kernel on the scenarios of tests/_poly_cases.py (certified and
# checked for richness on the oracle alone by tests/test_poly_host.py).
OPT, MAXIT, NOTCVX, INFEAS, NONFIN = 0, 1, 2, 3, 4
F64, F32 = torch.float64, torch.float32


def _tn(a, dev, dt=F64):
    return None if a is None else _t(a, dev, dt)


def _device_qp(c, dev, dt=F64, with_f=True):
    return batched.PolyQP(_t(oc.pack_lower(c.H), dev, dt), _tn(c.G, dev, dt),
                          _tn(c.F if with_f else None, dev, dt), _tn(c.lbz, dev, dt),
                          _tn(c.ubz, dev, dt))


def _host(z, y, st):
    torch.cuda.synchronize()
    return z.double().cpu().numpy(), y.double().cpu().numpy(), st.cpu().numpy()


def _solve_case(c, dev, dt=F64, **kw):
    """PolyQP.solve(x0, f1, hl, hu) of a case as float64 host arrays."""
    qp = _device_qp(c, dev, dt)
    return _host(*qp.solve(_tn(c.x0, dev, dt), _tn(c.f1, dev, dt), _tn(c.hl, dev, dt),
                           _tn(c.hu, dev, dt), **kw))


def _check_case(c, z, y, st, ztol, ytol, unique=True, only=None, eq_rows=(), fp32=False):
    """Instance by instance against the oracle: status OPTIMAL, z, y over all
    m_total rows (signs and box rows included; not the rows eq_rows), row and
    box feasibility.  Cases whose multipliers are not unique, and equality
    rows, get the KKT certificate of the device's (z, y) (_poly_cases.check_kkt)
    instead of the comparison of y.  Absolute tolerances of the feasibility
    and of the certificate: 1e-9 and 1e-8 * scale in fp64; in fp32 what the
    asserted z and y bounds allow a quantity that is exact at the reference to
    move: a row ztol max(1, |z_ref|) |C_r|_1, the stationarity residual
    ztol max(1, |z_ref|) |H|_inf + ytol max(1, |y_ref|) |C'|_inf.
    Returns the worst relative errors."""
    code = st & 0xFF
    worst_z = worst_y = 0.0
    C = c.qp.Call
    keep = np.array([r not in eq_rows for r in range(c.mt)])
    for i in (range(c.batch) if only is None else only):
        assert code[i] == OPT, (i, code)
        zr, yr, _ = c.ref[i]
        zs, ys = max(1.0, np.abs(zr).max()), max(1.0, np.abs(yr).max())
        ez = np.abs(z[i] - zr).max() / zs
        worst_z = max(worst_z, ez)
        assert ez < ztol, (i, ez)
        if unique:
            ey = np.abs(y[i] - yr)[keep].max(initial=0.0) / ys
            worst_y = max(worst_y, ey)
            assert ey < ytol, (i, ey)
        if fp32:
            feas = ztol * zs * np.abs(C).sum(axis=1)
            stat = ztol * zs * np.abs(c.H).sum(axis=1).max() + ytol * ys * np.abs(C).sum(axis=0).max()
        else:
            feas, stat = 1e-9, 1e-8 * c.scale(i)
        lo, hi = c.bounds(i)
        cz = C @ z[i]
        assert (cz - hi <= feas).all() and (lo - cz <= feas).all(), i
        if not unique or eq_rows:
            pc.check_kkt(c, i, z[i], y[i], stat, feas if fp32 else stat)
            rows = list(eq_rows)
            assert (np.abs(cz - hi)[rows] <= (feas[rows] if fp32 else feas)).all(), i
    return worst_z, worst_y


@pytest.mark.parametrize("n,m", pc.SHAPES_A)
def test_family_a_fp64(dev, n, m):
    """Every dual_range_kernel<double, BS>, BS = 1..8, through
    PolyQP.solve(x0, f1, hl, hu): prologue s0 = L x0 - Ut f1, two-sided rows
    with missing sides, a half-open box, epilogue Kt' x0 - Hinv f1 - Ut' y."""
    c = pc.family_a(n, m)
    assert (c.mt + 7) // 8 == pc.SHAPES_A.index((n, m)) + 1
    z, y, st = _solve_case(c, dev)
    wz, wy = _check_case(c, z, y, st, 1e-8, 1e-6)
    iters = (st >> 8) & 0xFFFF
    print(f"fp64 ({n}, {m}): worst relative error z {wz:.2e}, y {wy:.2e}; iterations {iters.tolist()}")
    assert (iters >= 2).any(), iters


# Worst relative error per shape of SHAPES_A of the fp32 kernels against the
# fp64 oracle on the fp32-rounded data, as measured on an MI355X (DESIGN.md
# section 3.4), z relative to max(1, |z_ref|) and y to max(1, |y_ref|); the
# bound is 10 x that with the floor 2e-4, the rule of test_fp32 in
# tests/test_gpu_poly_loop.py (the factor covers other seeds).
FP32_MEASURED = [1.9e-6, 1.6e-6, 4.7e-6, 2.6e-6, 1.3e-6, 8.1e-7, 8.2e-7, 1.7e-6]
FP32_MEASURED_Y = [2.9e-7, 5.9e-7, 1.7e-6, 2.3e-6, 8.3e-7, 1.7e-6, 1.6e-6, 2.1e-6]


def _bound32(measured):
    return max(2e-4, 10 * measured)


@pytest.mark.parametrize("n,m", pc.SHAPES_A)
def test_family_a_fp32(dev, n, m):
    """Every dual_range_kernel<float, BS>: the same checks at the fp32 bounds."""
    c = pc.family_a(n, m, fp32=True)
    k = pc.SHAPES_A.index((n, m))
    assert (c.mt + 7) // 8 == k + 1
    z, y, st = _solve_case(c, dev, F32)
    iters = (st >> 8) & 0xFFFF
    zb, yb = _bound32(FP32_MEASURED[k]), _bound32(FP32_MEASURED_Y[k])
    ez, ey = _check_case(c, z, y, st, np.inf, np.inf, fp32=True)
    print(f"fp32 ({n}, {m}): worst relative error z {ez:.3e} (bound {zb:.1e}), y {ey:.3e} "
          f"(bound {yb:.1e}); iterations {iters.tolist()}")
    _check_case(c, z, y, st, zb, yb, fp32=True)
    assert (iters >= 2).any(), iters


# Family B in fp32: measured worst relative errors (z, y) per case, bound as above
FP32_MEASURED_B = {"box_only": (3.6e-7, 4.5e-7), "scalar": (3.0e-8, 3.0e-8),
                   "scalar_box": (3.0e-8, 5.0e-8), "lower_only": (1.8e-7, 2.2e-7),
                   "project_zero": (7.4e-8, 4.4e-8), "equality": (6.6e-7, 3.7e-7)}


@pytest.mark.parametrize("name,fp32", [(k, False) for k in pc.CASES_B]
                         + [(k, True) for k, v in pc.CASES_B.items() if v[2]])
def test_family_b(dev, name, fp32):
    """m = 0, n = 1, lower sides only, the projection of 0, equality rows and
    dependent rows (compare z; certify the device's y by the KKT conditions)."""
    c = pc.family_b(name, fp32)
    unique = pc.CASES_B[name][1]
    z, y, st = _solve_case(c, dev, F32 if fp32 else F64)
    eq = pc.EQ_ROWS if name == "equality" else ()
    if fp32:
        zb, yb = (_bound32(v) for v in FP32_MEASURED_B[name])
        wz, wy = _check_case(c, z, y, st, np.inf, np.inf, eq_rows=eq, fp32=True)
        print(f"fp32 {name}: worst relative error z {wz:.3e} (bound {zb:.1e}), y {wy:.3e} "
              f"(bound {yb:.1e})")
        _check_case(c, z, y, st, zb, yb, eq_rows=eq, fp32=True)
        return
    wz, wy = _check_case(c, z, y, st, 1e-8, 1e-6, unique=unique, eq_rows=eq)
    iters = (st >> 8) & 0xFFFF
    print(f"fp64 {name}: worst relative error z {wz:.2e}, y {wy:.2e}; iterations {iters.tolist()}")
    if name == "scalar_box":
        # the last instance: the row is the most violated and goes in first, the
        # box row depends on it, so the row is dropped and the box row added
        assert iters[6] == 3 and y[6, 0] == 0 and y[6, 1] > 0
    if name == "project_zero":
        assert np.array_equal(c.f, np.zeros_like(c.f))


# ---------------------------------------------------- forms of the same call
def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _equal_bits(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_solve_poly_is_polyqp_solve(dev):
    """solve_poly(H, f, G, hl, hu, lbz, ubz) and PolyQP(H, G, None, lbz,
    ubz).solve(None, f, hl, hu) are the same launches: equal bit for bit."""
    c = pc.family_a(12, 20)
    f, hl, hu = _t(c.f, dev), _t(c.hl, dev), _t(c.hu, dev)
    a = batched.solve_poly(_t(oc.pack_lower(c.H), dev), f, _t(c.G, dev), hl, hu, _t(c.lbz, dev),
                           _t(c.ubz, dev))
    b = _device_qp(c, dev, with_f=False).solve(None, f, hl, hu)
    assert _equal_bits(a, b)
    _check_case(c, *_host(*a), 1e-8, 1e-6)


def test_x0_form_is_gradient_form(dev):
    """solve(x0, f1) against solve(None, F x0 + f1) with the gradient formed
    on the host: 1e-9, as in test_poly_parametric_x0."""
    c = pc.family_a(8, 11)
    qp = _device_qp(c, dev)
    hl, hu = _t(c.hl, dev), _t(c.hu, dev)
    z, y, st = _host(*qp.solve(_t(c.x0, dev), _t(c.f1, dev), hl, hu))
    z2, y2, st2 = _host(*qp.solve(None, _t(c.f, dev), hl, hu))
    assert (st & 0xFF == OPT).all() and (st2 & 0xFF == OPT).all()
    assert np.abs(z - z2).max() < 1e-9 and np.abs(y - y2).max() < 1e-9 * max(1.0, np.abs(y).max())


def test_shared_operands_are_broadcast(dev):
    """Stride 0: a shared (1-D) x0 and f with per-instance hl, hu, and
    per-instance x0 and f with shared hl, hu, equal the calls with the shared
    operand repeated per instance, bit for bit."""
    c = pc.family_a(6, 10)
    qp = _device_qp(c, dev)
    b = c.batch
    x0, f1, hl, hu = _t(c.x0, dev), _t(c.f1, dev), _t(c.hl, dev), _t(c.hu, dev)
    rep = lambda v: v.repeat(b, 1)  # noqa: E731
    a = qp.solve(x0[2], f1[2], hl, hu)
    assert a[0].shape == (b, c.n) and _equal_bits(a, qp.solve(rep(x0[2]), rep(f1[2]), hl, hu))
    a = qp.solve(x0, f1, hl[1], hu[1])
    assert _equal_bits(a, qp.solve(x0, f1, rep(hl[1]), rep(hu[1])))
    assert (batched.status_code(a[2]) == OPT).all()
    H, G, f = _t(oc.pack_lower(c.H), dev), _t(c.G, dev), _t(c.f, dev)
    a = batched.solve_poly(H, f[3], G, hl, hu, -0.7, 0.5)
    assert a[0].shape == (b, c.n) and _equal_bits(a, batched.solve_poly(H, rep(f[3]), G, hl, hu, -0.7, 0.5))
    a = batched.solve_poly(H, f, G, hl[4], hu[4], -0.7, 0.5)
    assert _equal_bits(a, batched.solve_poly(H, f, G, rep(hl[4]), rep(hu[4]), -0.7, 0.5))


def test_out_is_used_and_returned(dev):
    c = pc.family_a(6, 10)
    qp = _device_qp(c, dev)
    args = (_t(c.x0, dev), _t(c.f1, dev), _t(c.hl, dev), _t(c.hu, dev))
    ref = qp.solve(*args)
    out = (torch.full((c.batch, c.n), 7.0, dtype=F64, device=dev),
           torch.full((c.batch, c.mt), 7.0, dtype=F64, device=dev),
           torch.full((c.batch,), -1, dtype=torch.int32, device=dev))
    got = qp.solve(*args, out=out)
    assert all(g is o for g, o in zip(got, out)) and _equal_bits(got, ref)
    for o in out:
        o.fill_(7)
    sp = (_t(oc.pack_lower(c.H), dev), _t(c.f, dev), _t(c.G, dev), args[2], args[3],
          _t(c.lbz, dev), _t(c.ubz, dev))
    got = batched.solve_poly(*sp, out=out)
    assert all(g is o for g, o in zip(got, out)) and _equal_bits(got, batched.solve_poly(*sp))


def test_two_streams_share_the_workspace(dev):
    """The workspace is read-only during a solve: two solves of one PolyQP on
    two streams give the bits of the same two solves in sequence."""
    c = pc.family_a(24, 40)
    qp = _device_qp(c, dev)
    rep = 32
    a1 = tuple(_t(np.tile(v, (rep, 1)), dev) for v in (c.x0, c.f1, c.hl, c.hu))
    a2 = tuple(_t(np.tile(v[::-1], (rep, 1)), dev) for v in (c.x0, c.f1, c.hl, c.hu))
    seq = (qp.solve(*a1), qp.solve(*a2))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        r1 = qp.solve(*a1)
    with torch.cuda.stream(s2):
        r2 = qp.solve(*a2)
    torch.cuda.synchronize()
    assert _equal_bits(r1, seq[0]) and _equal_bits(r2, seq[1])
    assert (batched.status_code(r1[2]) == OPT).all() and (batched.status_code(r2[2]) == OPT).all()
    assert _equal_bits([r1[0][:c.batch]], [r1[0][-c.batch:]])


# ------------------------------------------------------------------ statuses
def _run_rows(qp, dev, x0, f1, hl, hu, **kw):
    return _host(*qp.solve(_tn(x0, dev), _tn(f1, dev), _tn(hl, dev), _tn(hu, dev), **kw))


def _spoil(c, name, bad):
    """(x0, f1, hl, hu) of a case with instance `bad` spoiled as `name` says."""
    x0, f1, hl, hu = c.x0.copy(), c.f1.copy(), c.hl.copy(), c.hu.copy()
    if name == "nan_f1":
        f1[bad, 3] = np.nan
    elif name == "inf_x0":
        x0[bad, 1] = np.inf
    elif name == "hl_above_hu":
        hl[bad, 1] = hu[bad, 1] + 1.0
    elif name == "hl_plus_inf":
        hl[bad, 6] = np.inf
    elif name == "hu_minus_inf":
        hu[bad, 3] = -np.inf
    elif name == "nan_f1_and_hl_above_hu":
        f1[bad, 0] = np.nan
        hl[bad, 1] = hu[bad, 1] + 1.0
    elif name == "nan_hl":
        hl[bad, 4] = np.nan
    elif name == "nan_hu":
        hu[bad, 4] = np.nan
    return x0, f1, hl, hu


SPOILED = [("nan_f1", NONFIN), ("inf_x0", NONFIN), ("hl_above_hu", INFEAS), ("hl_plus_inf", INFEAS),
           ("hu_minus_inf", INFEAS), ("nan_f1_and_hl_above_hu", NONFIN), ("nan_hl", INFEAS),
           ("nan_hu", INFEAS)]


def _check_bad_among_healthy(got, clean, bad, want):
    z, y, st = got
    assert (st & 0xFF)[bad] == want, st & 0xFF
    assert np.isnan(z[bad]).all() and np.isnan(y[bad]).all()
    keep = np.arange(len(st)) != bad
    for g, r in zip(got, clean):
        assert np.array_equal(g[keep], r[keep])
    assert ((st & 0xFF)[keep] == OPT).all()


def test_status_nonfinite_and_bound_check(dev):
    """One spoiled instance among healthy ones, each kind in a launch of its
    own: NONFINITE for a NaN in f1 or an Inf in x0 (also when a row has hl >
    hu: the kernel tests non-finite data first); INFEASIBLE for hl > hu, hl =
    +inf, hu = -inf and for a NaN row bound (!(hl <= hu) holds for a NaN).
    z and y of the spoiled instance are NaN; the neighbours keep the bits of
    the clean batch."""
    c = pc.family_a(12, 20)
    qp = _device_qp(c, dev)
    clean = _run_rows(qp, dev, c.x0, c.f1, c.hl, c.hu)
    assert (clean[2] & 0xFF == OPT).all()
    for k, (name, want) in enumerate(SPOILED):
        bad = k % c.batch
        _check_bad_among_healthy(_run_rows(qp, dev, *_spoil(c, name, bad)), clean, bad, want)


@pytest.mark.parametrize("side", ["lbz", "ubz"])
def test_status_nan_box_bound(dev, side):
    """A NaN entry in lbz or ubz (shared by the batch, so a PolyQP of its own):
    the same bound test, INFEASIBLE for every instance, z and y NaN."""
    c = pc.family_a(6, 10)
    box = {"lbz": c.lbz.copy(), "ubz": c.ubz.copy()}
    box[side][2] = np.nan
    qp = batched.PolyQP(_t(oc.pack_lower(c.H), dev), _t(c.G, dev), _t(c.F, dev),
                        _t(box["lbz"], dev), _t(box["ubz"], dev))
    z, y, st = _run_rows(qp, dev, c.x0, c.f1, c.hl, c.hu)
    assert (st & 0xFF == INFEAS).all(), st & 0xFF
    assert np.isnan(z).all() and np.isnan(y).all()


@pytest.mark.parametrize("box", [False, True])
def test_status_empty_polytope_by_ratio_test(dev, box):
    """Bounds that pass the bound check, but an empty polytope: two parallel
    rows sum z >= 1 and sum z <= -1, and a row sum z >= n ub + 1 that the box
    keeps out of reach.  The ratio test finds no step: INFEASIBLE."""
    rng = np.random.default_rng(41)
    n, b, bad = 4, 5, 2
    M = rng.normal(size=(n, n))
    H = M @ M.T / n + 0.5 * np.eye(n)
    f = rng.normal(size=(b, n))
    if box:
        G, ub = np.ones((1, n)), np.full(n, 0.5)
        hl, hu = np.full((b, 1), 1.0), None
        hl_bad = hl.copy()
        hl_bad[bad] = ub.sum() + 1.0
        hu_bad = None
    else:
        G, ub = np.ones((2, n)), None
        hl, hu = np.tile([1.0, -np.inf], (b, 1)), np.tile([np.inf, 3.0], (b, 1))
        hl_bad, hu_bad = hl.copy(), hu.copy()
        hu_bad[bad, 1] = -1.0
    healthy = pc.Case(H, G, None, None if ub is None else -ub, ub, None, f, hl, hu)
    qp = _device_qp(healthy, dev)
    clean = _run_rows(qp, dev, None, f, hl, hu)
    got = _run_rows(qp, dev, None, f, hl_bad, hu_bad)
    _check_bad_among_healthy(got, clean, bad, INFEAS)
    _check_case(healthy, *got, 1e-8, 1e-6, only=[i for i in range(b) if i != bad])


def test_status_not_convex_from_the_shared_inverse(dev):
    """H = diag(1, -1, 1, 1): the shared inverse meets a non-positive pivot and
    sets its flag; every instance ends NOT_CONVEX with NaN z and y."""
    n, b = 4, 3
    H = np.diag([1.0, -1.0, 1.0, 1.0])
    G = np.vstack([np.ones(n), np.arange(1.0, n + 1)])
    f = np.random.default_rng(2).normal(size=(b, n))
    for lbz in (None, -1.0):
        z, y, st = _host(*batched.solve_poly(_t(oc.pack_lower(H), dev), _t(f, dev), _t(G, dev),
                                             None, _t(np.ones(2), dev), lbz, None))
        assert (st & 0xFF == NOTCVX).all(), st & 0xFF
        assert np.isnan(z).all() and np.isnan(y).all()


def test_status_max_iter(dev):
    """max_iter = 1 on the (12, 20) instances and their scaled-down copies
    (tests/_poly_cases.maxiter_case): OPTIMAL and MAXITER only, and both; the
    iteration field at most 2; every z and y finite; the OPTIMAL ones are the
    oracle's."""
    c = pc.maxiter_case()
    z, y, st = _solve_case(c, dev, max_iter=1)
    code, iters = st & 0xFF, (st >> 8) & 0xFFFF
    print(f"max_iter=1: codes {code.tolist()}, iterations {iters.tolist()}")
    assert np.isin(code, (OPT, MAXIT)).all(), code
    assert (code == OPT).any() and (code == MAXIT).any()
    assert (code[:pc.BATCH_A] == MAXIT).all() and (code[-pc.BATCH_A:] == OPT).all()
    assert (iters <= 2).all()
    assert np.isfinite(z).all() and np.isfinite(y).all()
    _check_case(c, z, y, st, 1e-8, 1e-6, only=np.nonzero(code == OPT)[0])


def test_tol_argument(dev):
    """tol = 1e-6 (fp64): no instance takes more iterations than with the
    default tolerance, and every row holds to 1e-6 (1 + |bound|)."""
    c = pc.family_a(12, 20)
    _, _, st0 = _solve_case(c, dev)
    z, y, st = _solve_case(c, dev, tol=1e-6)
    assert (st & 0xFF == OPT).all() and (st0 & 0xFF == OPT).all()
    assert (((st >> 8) & 0xFFFF) <= ((st0 >> 8) & 0xFFFF)).all()
    for i in range(c.batch):
        lo, hi = c.bounds(i)
        cz = c.qp.Call @ z[i]
        fl, fu = np.isfinite(lo), np.isfinite(hi)
        assert ((lo - cz)[fl] <= 1e-6 * (1 + np.abs(lo[fl]))).all()
        assert ((cz - hi)[fu] <= 1e-6 * (1 + np.abs(hi[fu]))).all()


# -------------------------------------------------------------------- limits
def test_limit_m_total_65(dev):
    n, m = 5, 60
    H = _t(oc.pack_lower(np.eye(n)), dev)
    G, f, h = _t(np.ones((m, n)), dev), _t(np.zeros((2, n)), dev), _t(np.ones(m), dev)
    with pytest.raises(nat.MpcqpError, match="m_total=65"):
        batched.solve_poly(H, f, G, None, h, -1.0, 1.0)
    with pytest.raises(nat.MpcqpError, match="m_total=65"):
        batched.PolyQP(H, G, None, -1.0, 1.0)
    torch.cuda.synchronize()


def test_batch_zero_through_the_c_call(dev):
    c = pc.family_a(3, 2)
    qp = _device_qp(c, dev)
    z = torch.full((1, c.n), 7.0, dtype=F64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = nat.load().mpcqp_poly_solve(nat.F64, 0, c.n, c.m, 1, c.nx, qp.ws.data_ptr(), None, 0, None,
                                     0, None, None, 0, qp.lbz.data_ptr(), qp.ubz.data_ptr(),
                                     z.data_ptr(), None, st.data_ptr(), 0, 0.0, None)
    torch.cuda.synchronize()
    assert rc == 0 and (z == 7.0).all() and (st == -1).all()


# ---------------------------------------------------------------- validation
def test_wrapper_validation(dev):
    """PolyQP.solve and solve_poly refuse malformed operands with their own
    ValueError before any launch (hl and hu of different kinds used to give
    the kernel a wrong row stride)."""
    c = pc.family_a(6, 10)
    n, m, b = c.n, c.m, c.batch
    H, G, F = _t(oc.pack_lower(c.H), dev), _t(c.G, dev), _t(c.F, dev)
    x0, f1, f, hl, hu = (_t(v, dev) for v in (c.x0, c.f1, c.f, c.hl, c.hu))
    qp = batched.PolyQP(H, G, F, -0.7, 0.5)
    ok = qp.solve(x0, f1, hl, hu)
    both = "both be shared or both per instance"

    def bad(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            qp.solve(*a, **kw)

    def bad_sp(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            batched.solve_poly(*a, **kw)

    bad(both, x0, f1, hl, hu[0])
    bad(both, x0, f1, hl[0], hu)
    bad_sp(both, H, f, G, hl, hu[0])
    bad_sp(both, H, f, G, hl[0], hu)
    bad("different batch sizes", x0, f1, hl, hu[:3])
    bad(f"hl must be \\({m},\\)", x0, f1, hl[:, :m - 1], hu)
    bad(f"hu must be \\({m},\\)", x0, f1, hl, hu[0, :m - 1])
    bad_sp(f"hl must be \\({m},\\)", H, f, G, hl[:, 1:], hu)
    bad_sp(f"hu must be \\({m},\\)", H, f, G, None, hu.reshape(b, m, 1))
    bad(f"f must be \\({n},\\)", x0, f1[:, :n - 1], hl, hu)
    bad_sp("H must be packed lower", H, f[:, :n - 1], G[:, :n - 1], hl, hu)
    bad(f"x0 must be \\({c.nx},\\)", x0[:, :2], f1, hl, hu)
    bad(f"x0 must be \\({c.nx},\\)", x0.reshape(b, c.nx, 1), f1, hl, hu)
    bad("inconsistent batch sizes", x0[:4], f1, hl, hu)
    with pytest.raises(ValueError, match="no x0 -> gradient map F"):
        batched.PolyQP(H, G, None, -0.7, 0.5).solve(x0, f1, hl, hu)
    with pytest.raises(ValueError, match=f"G must be \\(m, {n}\\)"):
        batched.PolyQP(H, G[:, :n - 1], F)
    bad_sp(f"G must be \\(m, {n}\\)", H, f, G[:, :n - 1].contiguous(), hl, hu)
    with pytest.raises(ValueError, match=f"F must be \\({n}, nx\\)"):
        batched.PolyQP(H, G, F[:n - 1])
    for v in (torch.zeros((b, n), dtype=F64, device=dev), torch.zeros(n + 1, dtype=F64, device=dev)):
        with pytest.raises(ValueError, match="lbz must be a scalar or"):
            batched.PolyQP(H, G, F, v, None)
        bad_sp("ubz must be a scalar or", H, f, G, hl, hu, None, v)
    good = [torch.empty_like(t) for t in ok]
    bad("out must be a triple", x0, f1, hl, hu, out=good[:2])
    spoilt = {"z": (0, torch.empty((b, n + 1), dtype=F64, device=dev)),
              "y": (1, torch.empty((b, c.mt), dtype=F32, device=dev)),
              "status": (2, torch.empty((b,), dtype=torch.int64, device=dev))}
    for name, (k, t) in spoilt.items():
        out = list(good)
        out[k] = t
        bad(f"out {name} must be a contiguous", x0, f1, hl, hu, out=tuple(out))
        bad_sp(f"out {name} must be a contiguous", H, f, G, hl, hu, -0.7, 0.5, out=tuple(out))
    out = list(good)
    out[0] = torch.empty((n, b), dtype=F64, device=dev).t()
    bad("out z must be a contiguous", x0, f1, hl, hu, out=tuple(out))
    out[0] = torch.empty((b, n), dtype=F64)
    bad("out z must be a contiguous", x0, f1, hl, hu, out=tuple(out))
    assert _equal_bits(qp.solve(x0, f1, hl, hu, out=tuple(good)), ok)
