"""CPU: the reverse-time recursion of the polytope-loop adjoint
(tests/_poly_loop_vjp_cases.py) against central differences of the oracle's
closed loop, the binding of include/mpcqp_poly_loop_diff.h and the argument
checks of mpcqp_mpc_poly_loop_vjp, which run before any device work.

Central differences with eps = 1e-6 through _poly_loop_cases.LoopQP
(oracle.qp.poly_qp per step, KKT-certified), L a fixed random linear function
of xs, us, zs and ys.  The bound is 1e-6 relative to 1 + max|grad| of the
instance, that of tests/test_poly_vjp_host.py at the same eps; every reference
episode is asserted feasible with active sets separated by 1e-5, so the step
stays inside them.  Worst disagreement measured: 4.6e-9 over SHAPES[:6] (all
groups), 2.5e-8 for the session problem at N = 5, 4.1e-9 on the drift prefix,
2.0e-8 at config 4.  The session problem at N = 10 is left out of the
difference check: its ill-conditioned H brings the differences themselves to
5e-7, half the bound.
"""
import ctypes

import numpy as np
import pytest

import _poly_loop_cases as lc
import _poly_loop_vjp_cases as lv
from model_predictive_control_amd import _native as nat
from test_condense_vjp_host import _ctypes_kind, _prototypes   # the header parser of that test

EPS = 1e-6
TOL = 1e-6         # relative to 1 + max|grad|
SEPARATION = 1e-5  # of every reference episode's active sets


def _variant(qp, **over):
    """qp with some of E, hl, hu, lbz, ubz, A, B replaced."""
    get = lambda k: over.get(k, getattr(qp, k))  # noqa: E731
    return lc.LoopQP(qp.H, qp.F, qp.G if qp.m else None, get("E"), get("hl"), get("hu"),
                     get("lbz") if qp.nbox else None, get("ubz") if qp.nbox else None,
                     get("A"), get("B"))


def _loss(qp, x0_base, w_base, up, **over):
    x0 = over.pop("x0", x0_base)
    w = over.pop("w", w_base)
    q = _variant(qp, **over) if over else qp
    xs, zs, ys = lv.episode(q, x0, up[1].shape[0], w=w)
    return lv.loss(xs, zs, ys, qp.nu, *up)


def _fd(qp, x0, w, up, name, x, mask=None):
    """Central differences of the loss in the entries of operand ``name`` (those
    of ``mask``)."""
    out = np.zeros(x.shape)
    for k in np.ndindex(*x.shape):
        if mask is not None and not mask[k]:
            continue
        d = np.zeros(x.shape)
        d[k] = EPS
        out[k] = (_loss(qp, x0, w, up, **{name: x + d}) - _loss(qp, x0, w, up, **{name: x - d})) / (2 * EPS)
    return out


def _check(qp, x0, T, w=None, groups=("x0", "w", "A", "B", "E", "hl", "hu", "lbz", "ubz"), seed=0,
           held_only=False):
    """Worst relative disagreement between the recursion and central differences
    for one instance, over ``groups``; also the episode (for the assertions on
    the reference).  ``held_only``: of hu only the rows held at some step are
    differenced (n = 200: a solve is slow); on the others the recursion's entry
    must be an exact zero, which is what a bound that is never met gives."""
    xs, zs, ys = lv.episode(qp, x0, T, w=w)
    up = lv.upstream(T, qp.nx, qp.nu, qp.n, qp.mt, seed)
    r = lv.recursion(qp, xs, zs, ys, *up)
    m = qp.m
    wz = np.zeros((T, qp.nx)) if w is None else w
    hu_rows = np.isfinite(qp.hu)
    if held_only:
        hu_rows &= (ys[:, :m] > 0).any(axis=0)
        assert hu_rows.any() and not r["ghu"][:m][~hu_rows].any()
    table = dict(
        x0=lambda: (r["gx0"], _fd(qp, x0, wz, up, "x0", x0)),
        w=lambda: (r["gw"], _fd(qp, x0, wz, up, "w", wz)),
        A=lambda: (r["gA"], _fd(qp, x0, wz, up, "A", qp.A)),
        B=lambda: (r["gB"], _fd(qp, x0, wz, up, "B", qp.B)),
        E=lambda: (r["gE"], _fd(qp, x0, wz, up, "E", qp.E)),
        hl=lambda: (r["ghl"][:m], _fd(qp, x0, wz, up, "hl", qp.hl, np.isfinite(qp.hl))),
        hu=lambda: (r["ghu"][:m], _fd(qp, x0, wz, up, "hu", qp.hu, hu_rows)),
        lbz=lambda: (r["ghl"][m:], _fd(qp, x0, wz, up, "lbz", qp.lbz, np.isfinite(qp.lbz))),
        ubz=lambda: (r["ghu"][m:], _fd(qp, x0, wz, up, "ubz", qp.ubz, np.isfinite(qp.ubz))))
    pairs = [table[k]() for k in groups if not (k == "E" and qp.E is None)
             and not (k in ("lbz", "ubz") and not qp.nbox)]
    # a bound that is infinite cannot be active: its entry is an exact zero
    assert not r["ghl"][:m][~np.isfinite(qp.hl)].any() and not r["ghu"][:m][~np.isfinite(qp.hu)].any()
    scale = 1 + max(float(np.abs(an).max()) for an, _ in pairs)
    worst = max(float(np.abs(an - fd).max()) / scale for an, fd in pairs)
    return worst, (xs, zs, ys)


def _sets(ys):
    return np.sign(ys).astype(int)


@pytest.mark.parametrize("nx,nu,N", lc.SHAPES[:6])
def test_recursion_vs_central_differences_shapes(nx, nu, N):
    """Every group at every instance of the first six shapes, T = 6."""
    p = lc.shape_problem(nx, nu, N)
    qp = p["qp"]
    worst, changes, active = 0.0, False, False
    for i in range(lc.SHAPE_B):
        assert p["ref"][i][3] is None            # the oracle's loop is feasible at every step
        err, (xs, zs, ys) = _check(qp, p["x0"][i], lc.SHAPE_T)
        assert lv.separation(qp, xs, zs, ys) >= SEPARATION, (i, lv.separation(qp, xs, zs, ys))
        s = _sets(ys)
        active |= bool(s.any())
        changes |= bool((s[1:] != s[:-1]).any())
        worst = max(worst, err)
    print(f"({nx},{nu},{N}): worst relative disagreement {worst:.2e}")
    assert active and changes
    assert worst <= TOL, worst


def test_recursion_vs_central_differences_session():
    """Session-2 Problem at N = 5, the seven X0_SESSION, T = 12: dL/dx0 and every
    bound row.  Both sides are active, some instance is active at every step, and
    some instance's set changes between consecutive steps."""
    qp, ref = lc.session_reference("Problem", 5)
    T = lc.T_EPISODE
    worst, sets = 0.0, []
    for i, x0 in enumerate(lc.X0_SESSION):
        assert ref[i][3] is None
        err, (xs, zs, ys) = _check(qp, x0, T, groups=("x0", "hl", "hu", "lbz", "ubz"), seed=i)
        assert lv.separation(qp, xs, zs, ys) >= SEPARATION, (i, lv.separation(qp, xs, zs, ys))
        sets.append(_sets(ys))
        worst = max(worst, err)
    sets = np.stack(sets)                          # (7, T, mt)
    assert (sets > 0).any() and (sets < 0).any()
    assert (sets != 0).any(axis=2).any(axis=0).all()
    assert (sets[:, 1:] != sets[:, :-1]).any()
    print(f"session N=5: worst relative disagreement {worst:.2e}")
    assert worst <= TOL, worst


def test_recursion_vs_central_differences_drift():
    """20 steps of the drift scenario: the disturbance w pushes the position
    against p_max."""
    qp, w, ref = lc.drift_reference()
    T = 20
    worst = 0.0
    for i in range(2):
        assert ref[i][3] is None
        err, (xs, zs, ys) = _check(qp, np.zeros(2), T, w=w[:T, i],
                                   groups=("x0", "w", "hl", "hu", "lbz", "ubz"), seed=i)
        assert lv.separation(qp, xs, zs, ys) >= SEPARATION
        worst = max(worst, err)
    print(f"drift: worst relative disagreement {worst:.2e}")
    assert worst <= TOL, worst


def test_recursion_vs_central_differences_config4():
    """BASELINE config 4 as a loop (n = 200, 40 one-sided rows, no box, E = None):
    dL/dx0 and the finite bound rows."""
    p = lc.config4_problem()
    qp = p["qp"]
    assert qp.E is None and not qp.nbox and qp.n == 200
    worst, active = 0.0, False
    for i in range(lc.SHAPE_B):
        assert p["ref"][i][3] is None
        err, (xs, zs, ys) = _check(qp, p["x0"][i], lc.SHAPE_T, groups=("x0", "hu"), held_only=True)
        assert lv.separation(qp, xs, zs, ys) >= SEPARATION, (i, lv.separation(qp, xs, zs, ys))
        active |= bool(ys.any())
        worst = max(worst, err)
    print(f"config 4: worst relative disagreement {worst:.2e}")
    assert active
    assert worst <= TOL, worst


# ------------------------------------------------------------------- the ABI
NAMES = {"mpcqp_mpc_poly_loop_vjp", "mpcqp_mpc_poly_loop_vjp_workspace"}


def test_binding_matches_the_header():
    protos = _prototypes("mpcqp_poly_loop_diff.h")
    assert set(protos) == set(nat.SIGNATURES_POLY_LOOP_DIFF) == NAMES
    for name, proto in protos.items():
        res, args = nat.SIGNATURES_POLY_LOOP_DIFF[name]
        assert (_ctypes_kind(res), [_ctypes_kind(t) for t in args]) == proto, name
    assert len(protos["mpcqp_mpc_poly_loop_vjp"][1]) == 28
    assert protos["mpcqp_mpc_poly_loop_vjp_workspace"] == ("size", ["i32"] * 6)
    tables = [set(nat.SIGNATURES), set(nat.SIGNATURES_DIFF), set(nat.SIGNATURES_POLY_DIFF),
              set(nat.SIGNATURES_POLY_LOOP_DIFF)]
    for i in range(4):
        for j in range(i):
            assert not tables[i] & tables[j], (i, j)
    assert nat.ABI_VERSION == 1
    lib = nat.load()
    for name in protos:
        assert hasattr(lib, name), name


def test_workspace_size():
    lib = nat.load()
    a256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for dtype, es in ((nat.F64, 8), (nat.F32, 4)):
        for batch, n, m, nbox, steps in ((1, 3, 2, 1, 1), (5, 14, 42, 1, 6), (4096, 200, 40, 0, 50),
                                         (3, 5, 10, 1, 0)):
            mt = m + (n if nbox else 0)
            rows = batch * steps
            want = a256(a256(rows * n * es) + rows * mt * es)
            assert lib.mpcqp_mpc_poly_loop_vjp_workspace(dtype, batch, n, m, nbox, steps) == want
    assert lib.mpcqp_mpc_poly_loop_vjp_workspace(nat.F64, 4, 60, 5, 1, 3) == 0   # m_total = 65
    assert lib.mpcqp_mpc_poly_loop_vjp_workspace(7, 4, 3, 2, 1, 3) == 0
    assert lib.mpcqp_mpc_poly_loop_vjp_workspace(nat.F64, 4, 3, 2, 1, -1) == 0
    assert lib.mpcqp_mpc_poly_loop_vjp_workspace(nat.F64, -1, 3, 2, 1, 3) == 0
    assert lib.mpcqp_mpc_poly_loop_vjp_workspace(nat.F64, 4, 0, 2, 0, 3) == 0


def _call(lib, *, dtype=nat.F64, batch=4, n=6, m=10, nbox=1, nx=3, nu=2, steps=5, ptr=True,
          ys=True, A=True, vstatus=True, gzs=True, scratch=None):
    """mpcqp_mpc_poly_loop_vjp with dummy pointers (never dereferenced: every
    call here fails in the argument checks or has batch = 0)."""
    one = ctypes.c_void_p(1) if ptr else None
    need = lib.mpcqp_mpc_poly_loop_vjp_workspace(dtype, batch, n, m, nbox, steps)
    return lib.mpcqp_mpc_poly_loop_vjp(
        dtype, batch, n, m, nbox, nx, nu, steps, one, one, one if A else None, one,
        one if ys else None, None, one, one, one if gzs else None, one, one, one, one, one, one, one,
        one if vstatus else None, one, need if scratch is None else scratch, None)


def test_argument_checks():
    lib = nat.load()
    err = lib.mpcqp_last_error
    name = b"mpcqp_mpc_poly_loop_vjp"
    assert _call(lib, dtype=7) == -1 and b"dtype" in err() and name in err()
    assert _call(lib, n=25, m=40) == -1 and b"m_total=65" in err() and name in err()
    assert _call(lib, m=0, nbox=0) == -1 and b"m_total=0" in err() and name in err()
    assert _call(lib, nx=17) == -1 and b"nx=17" in err() and name in err()
    assert _call(lib, nx=0) == -1 and b"nx=0" in err() and name in err()
    assert _call(lib, nu=0) == -1 and b"nu=0" in err() and name in err()
    assert _call(lib, nu=7) == -1 and b"nu=7" in err() and name in err()      # nu > n
    assert _call(lib, nu=17, n=20, m=2) == -1 and b"nu=17" in err() and name in err()
    assert _call(lib, ys=False) == -1 and b"ys" in err() and name in err()
    assert _call(lib, A=False) == -1 and b"required" in err() and name in err()
    assert _call(lib, vstatus=False) == -1 and b"required" in err() and name in err()
    need = lib.mpcqp_mpc_poly_loop_vjp_workspace(nat.F64, 4, 6, 10, 1, 5)
    assert need > 0
    assert _call(lib, scratch=need - 1) == -1 and b"scratch" in err() and name in err()
    assert _call(lib, batch=-1) == -1 and b"batch" in err() and name in err()
    assert _call(lib, steps=-1) == -1 and b"steps" in err() and name in err()
    assert _call(lib, n=0) == -1 and name in err()
    assert _call(lib, m=-1) == -1 and name in err()
    assert _call(lib, batch=0) == 0
    assert _call(lib, batch=0, ptr=False) == 0
    assert _call(lib, batch=0, scratch=0) == 0
