"""GPU: the adjoint kernel of condensing (mpcqp_condense_vjp,
include/mpcqp_diff.h) against the NumPy closed form of
tests/_condense_vjp_cases.py, its status rule, graph capture, and the autograd
functions built on it (condense_diff, mpc_box_model_diff,
mpc_box_loop_model_diff).

Errors are max|device - reference| / (1 + max|reference|) per output array,
against the fp64 closed form on data rounded to the dtype under test.
Tolerances: ten times the largest such error measured over every case of
test_kernel_vs_closed_form (printed by the test itself):
  fp64  measured 1.406e-15 (at (4, 1, 32); 2.0e-16, 3.1e-16, 6.8e-16, 8.1e-16,
        5.2e-16, 1.2e-15 at (1, 1, 1), (4, 2, 1), (2, 1, 3), (2, 1, 20), (3, 2, 4),
        (4, 2, 16)), so the tolerance 1.406e-14 is under the ceiling 1e-9;
  fp32  measured 7.096e-7 (at (4, 2, 16); 8.1e-8, 1.1e-7, 1.7e-7, 4.6e-7, 2.2e-7,
        5.0e-7 at the others in the order of SHAPES) against the fp64 closed form
        on fp32-rounded data: tolerance 7.096e-6, under the ceiling 1e-4.
condense_diff and mpc_box_model_diff hold the fp64 tolerance: mpc_box_model_diff
against mpc_box_diff measured 6.6e-16, its A, B, c gradients against the composed
closed forms 1.4e-15.  The episode test's bound is TOL_EPISODE below; measured
1.3e-14 (plant=None) and 1.6e-14 (plant=(Ap, Bp)).
"""
import ctypes

import numpy as np
import pytest
import torch

import _box_loop_vjp_cases as lc
import _box_vjp_cases as vc
import _condense_vjp_cases as cv
from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import autograd as ag
from model_predictive_control_amd import batched
from model_predictive_control_amd.condense_diff import condense_vjp
from oracle import condense as oc

pytestmark = pytest.mark.gpu

MEASURED_F64 = 1.406e-15
MEASURED_F32 = 7.096e-7
TOL_F64 = 10 * MEASURED_F64
TOL_F32 = 10 * MEASURED_F32
CEILING_F64, CEILING_F32 = 1e-9, 1e-4
# The episode test compares gradients that the loop adjoint (mpcqp_mpc_box_loop_vjp)
# computes first -- the plant's gA, gB as they are, the model's from its gH, gF --
# so its bound is that kernel's own tolerance against the same closed form (the
# fp64 tolerance of tests/test_gpu_box_loop_vjp.py, ten times its measured
# 1.088e-14) plus this kernel's.
TOL_EPISODE = 10 * 1.088e-14 + TOL_F64
OUTS = cv.OUTPUTS
UPS = ("gH", "gF", "gf")
B = cv.BATCH
NAN = float("nan")
F64 = torch.float64


def _t(a, dev, dt=F64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(a, b):
    """Equal bit for bit (the sign of a zero included)."""
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _npdt(dt):
    return np.float64 if dt == F64 else np.float32


def _device(p, dev, dt):
    return {k: _t(v, dev, dt) for k, v in p.items()}


def _raw(t, nx, nu, N, tv, *, shared=False, c=True, x0=True, ups=UPS, outs=OUTS + ("vstatus",)):
    """mpcqp_condense_vjp as it is on the device scenario ``t``: per-instance
    inputs, or instance 0's with stride 0; only the upstream gradients in
    ``ups`` and the outputs in ``outs`` passed (the rest NULL); the outputs
    pre-filled with NaN / -1 so that an entry the kernel leaves out shows."""
    dt, dev = t["A"].dtype, t["A"].device
    S = (N,) if tv else ()
    shapes = dict(gA=(B, *S, nx, nx), gB=(B, *S, nx, nu), gQ=(B, nx, nx), gR=(B, nu, nu),
                  gQf=(B, nx, nx), gc=(B, N, nx), gx0=(B, nx))
    o = {k: torch.full(shapes[k], NAN, dtype=dt, device=dev) for k in outs if k != "vstatus"}
    if "vstatus" in outs:
        o["vstatus"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    p = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731
    head = []
    for k in ("A", "B", "Q", "R", "Qf", "c", "x0"):
        use = (k != "c" or c) and (k != "x0" or x0)
        head += [p(t[k]) if use else None, 0 if shared or not use else int(t[k][0].numel())]
    rc = nat.load().mpcqp_condense_vjp(
        nat.F64 if dt == F64 else nat.F32, B, nx, nu, N, nat.TV if tv else 0, *head,
        *(p(t[k]) if k in ups else None for k in UPS), *(p(o.get(k)) for k in OUTS),
        p(o.get("vstatus")), torch.cuda.current_stream().cuda_stream)
    nat.check(rc, "mpcqp_condense_vjp")
    torch.cuda.synchronize()
    return o


def _reference(p, N, **kw):
    cf = [cv.reference(p, N, i, **kw) for i in range(B)]
    return {k: np.stack([r[k] for r in cf]) for k in OUTS}


# what is given and what is asked for: (c, x0, upstream gradients, outputs)
ALL = OUTS + ("vstatus",)
VARIANTS = [
    (True, True, UPS, ALL),
    (False, True, UPS, ALL),
    (True, False, UPS, ALL),
    (False, False, UPS, ALL),
    (True, True, ("gH",), ALL),
    (True, True, ("gF",), ALL),
    (True, True, ("gf",), ALL),
    (True, True, UPS, ("gA", "gc")),
    (True, True, UPS, ("gB", "gQ", "gx0")),
    (False, True, UPS, ("gQf", "gR", "vstatus")),
]
SHAPE_DT = [(s, F64) for s in cv.SHAPES] + [(s, torch.float32) for s in cv.SHAPES]
SHAPE_DT_IDS = [f"nx{s[0]}nu{s[1]}N{s[2]}-{'f64' if dt == F64 else 'f32'}" for s, dt in SHAPE_DT]


@pytest.mark.parametrize("shape,dt", SHAPE_DT, ids=SHAPE_DT_IDS)
def test_kernel_vs_closed_form(dev, shape, dt):
    """Time-invariant and MPCQP_TV, per-instance inputs and instance 0's with
    stride 0, batch 7 (seven wavefronts), every variant of VARIANTS: with and
    without c, x0 NULL, each upstream gradient alone, output subsets.

    Measured, worst over the 40 cases of a shape, in the order of SHAPES: fp64
    1.976e-16, 3.064e-16, 6.764e-16, 8.060e-16, 5.191e-16, 1.152e-15, 1.406e-15;
    fp32 8.064e-8, 1.103e-7, 1.672e-7, 4.597e-7, 2.159e-7, 7.096e-7, 4.988e-7."""
    nx, nu, N = shape
    worst = 0.0
    for tv in (False, True):
        p = cv.scenario(nx, nu, N, tv, _npdt(dt))
        t = _device(p, dev, dt)
        for shared in (False, True):
            for c, x0, ups, outs in VARIANTS:
                o = _raw(t, nx, nu, N, tv, shared=shared, c=c, x0=x0, ups=ups, outs=outs)
                assert set(o) == set(outs)
                if "vstatus" in outs:
                    assert (o["vstatus"] == 0).all(), o["vstatus"]
                ref = _reference(p, N, c=c, x0=x0, ups=ups, shared=shared)
                for k in outs:
                    if k == "vstatus":
                        continue
                    got = _np(o[k])
                    assert got.shape == ref[k].shape, k
                    assert np.isfinite(got).all(), (k, tv, shared, c, x0, ups)
                    worst = max(worst, cv.rel_err(got, ref[k]))
                for k in set(outs) & {"gQ", "gR", "gQf"}:
                    assert _bits(o[k], o[k].transpose(-1, -2).contiguous()), k
    print(f"{shape} {dt}: worst relative error {worst:.3e}")
    assert TOL_F64 <= CEILING_F64 and TOL_F32 <= CEILING_F32
    assert worst <= (TOL_F64 if dt == F64 else TOL_F32), worst


@pytest.mark.parametrize("tv", [False, True], ids=["lti", "tv"])
@pytest.mark.parametrize("where", ["A", "c", "gF"])
def test_nonfinite_gives_zeros(dev, where, tv):
    """A NaN in one instance's A, c or gF: NONFINITE and exact zeros for that
    instance; the others equal the clean run bit for bit."""
    nx, nu, N = 3, 2, 4
    p = cv.scenario(nx, nu, N, tv)
    t = _device(p, dev, F64)
    clean = _raw(t, nx, nu, N, tv)
    assert (clean["vstatus"] == 0).all()
    for bad in (0, 3, B - 1):
        t2 = dict(t)
        t2[where] = t[where].clone()
        t2[where][bad].view(-1)[-1] = NAN if bad else float("inf")
        o = _raw(t2, nx, nu, N, tv)
        others = [i for i in range(B) if i != bad]
        assert int(o["vstatus"][bad]) == nat.STATUS_NONFINITE
        assert (o["vstatus"][others] == 0).all()
        for k in OUTS:
            assert _bits(o[k][bad], torch.zeros_like(o[k][bad])), k
            assert _bits(o[k][others], clean[k][others]), k
    # an unused input may hold anything
    t2 = dict(t)
    t2["c"] = torch.full_like(t["c"], NAN)
    o = _raw(t2, nx, nu, N, tv, c=False)
    ref = _raw(t, nx, nu, N, tv, c=False)
    for k in ALL:
        assert _bits(o[k], ref[k]), k


def test_wrapper_sums_shared_inputs_through_a_select(dev):
    """condense_diff.condense_vjp: a shared plant's gradients are the sum of
    the per-instance ones, a failed instance adding an exact zero."""
    nx, nu, N = 2, 1, 20
    p = cv.scenario(nx, nu, N, False)
    t = _device(p, dev, F64)
    sh = {k: t[k][0] for k in ("A", "B", "Q", "R", "Qf", "c")}
    ups = {k: t[k] for k in UPS}
    r = condense_vjp(sh["A"], sh["B"], sh["Q"], sh["R"], sh["Qf"], N, t["x0"], sh["c"], **ups)
    cf = [cv.closed_form(p["A"][0], p["B"][0], p["Q"][0], p["R"][0], p["Qf"][0], N, x0=p["x0"][i],
                         c=p["c"][0], gH=p["gH"][i], gF=p["gF"][i], gf=p["gf"][i]) for i in range(B)]
    ref = {k: np.stack([c[k] for c in cf]) for k in OUTS}
    for k in ("gA", "gB", "gQ", "gR", "gQf", "gc"):
        assert r[k].shape == ref[k].shape[1:], k
        assert cv.rel_err(_np(r[k]), ref[k].sum(0)) <= TOL_F64, k
    assert cv.rel_err(_np(r["gx0"]), ref["gx0"]) <= TOL_F64
    ups["gf"] = t["gf"].clone()
    ups["gf"][2, 0] = NAN
    r2 = condense_vjp(sh["A"], sh["B"], sh["Q"], sh["R"], sh["Qf"], N, t["x0"], sh["c"], **ups)
    assert r2["vstatus"].tolist() == [0, 0, nat.STATUS_NONFINITE, 0, 0, 0, 0]
    keep = [i for i in range(B) if i != 2]
    for k in ("gA", "gB", "gQ", "gR", "gQf", "gc"):
        assert torch.isfinite(r2[k]).all(), k
        assert cv.rel_err(_np(r2[k]), ref[k][keep].sum(0)) <= TOL_F64, k
    assert (r2["gx0"][2] == 0).all()
    with pytest.raises(ValueError):
        condense_vjp(sh["A"], sh["B"], sh["Q"], sh["R"], sh["Qf"], N, need=("gH",))
    with pytest.raises(ValueError):
        condense_vjp(sh["A"], sh["B"], sh["Q"], sh["R"], sh["Qf"], N, gF=t["gf"])
    o = condense_vjp(sh["A"], sh["B"], sh["Q"], sh["R"], sh["Qf"], N, gH=t["gH"], need=("gA",))
    assert o["gB"] is None and o["gA"].shape == (nx, nx) and o["vstatus"].shape == (B,)


def test_graph_capture_condense_and_adjoint(dev):
    """batched.condense and the adjoint captured in one HIP graph on one stream:
    two replays give the eager bits."""
    nx, nu, N = 4, 2, 16
    p = cv.scenario(nx, nu, N, True)
    t = _device(p, dev, F64)

    def run():
        cd = batched.condense(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, x0=t["x0"], c=t["c"],
                              tv=True, outputs=("H", "F", "f"))
        # the condensed problem itself as the upstream gradient: the adjoint reads the forward
        o = condense_vjp(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], t["c"], tv=True,
                         gH=cd["H"], gF=cd["F"], gf=cd["f"])
        return [cd["H"], cd["F"], cd["f"]] + [o[k] for k in ALL]

    eager = [v.clone() for v in run()]
    assert (eager[-1] == 0).all()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for v in out:
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(out, eager):
            assert _bits(a, e)


# ------------------------------------------------------------ condense_diff
INPUTS = ("A", "B", "Q", "R", "Qf", "x0", "c")
GNAME = dict(A="gA", B="gB", Q="gQ", R="gR", Qf="gQf", x0="gx0", c="gc")


@pytest.mark.parametrize("tv", [False, True], ids=["lti", "tv"])
def test_condense_diff_values_and_gradients(dev, tv):
    nx, nu, N = 3, 2, 4
    p = cv.scenario(nx, nu, N, tv)
    t = _device(p, dev, F64)
    a = {k: t[k].clone().requires_grad_(True) for k in INPUTS}
    H, F, f = ag.condense_diff(a["A"], a["B"], a["Q"], a["R"], a["Qf"], N, a["x0"], a["c"], tv=tv)
    cd = batched.condense(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, x0=t["x0"], c=t["c"], tv=tv,
                          outputs=("H", "F", "f"))
    assert _bits(H.detach(), cd["H"]) and _bits(F.detach(), cd["F"]) and _bits(f.detach(), cd["f"])
    L = (t["gH"] * H).sum() + (t["gF"] * F).sum() + (t["gf"] * f).sum()
    got = dict(zip(INPUTS, torch.autograd.grad(L, [a[k] for k in INPUTS])))
    ref = _reference(p, N)
    for k in INPUTS:
        assert got[k].shape == a[k].shape, k
        assert cv.rel_err(_np(got[k]), ref[GNAME[k]]) <= TOL_F64, k
    # one output alone, in the order asked for
    F2, H2 = ag.condense_diff(a["A"], a["B"], a["Q"], a["R"], a["Qf"], N, tv=tv, outputs=("F", "H"))
    cd2 = batched.condense(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, tv=tv, outputs=("F", "H"))
    assert _bits(F2.detach(), cd2["F"]) and _bits(H2.detach(), cd2["H"])
    gA, = torch.autograd.grad((t["gF"] * F2).sum(), [a["A"]])
    refF = _reference(p, N, c=False, x0=False, ups=("gF",))
    assert cv.rel_err(_np(gA), refF["gA"]) <= TOL_F64
    with pytest.raises(ValueError):
        ag.condense_diff(a["A"], a["B"], a["Q"], a["R"], a["Qf"], N, tv=tv, outputs=("Gam",))


def test_condense_diff_shared_plant_and_forms_of_R(dev):
    """A shared plant with per-instance x0: the gradients are summed over the
    batch.  R as a scalar gets the trace of the matrix gradient, R as a vector
    its diagonal."""
    nx, nu, N = 4, 2, 16
    p = cv.scenario(nx, nu, N, False)
    t = _device(p, dev, F64)
    r = np.array([0.7, 1.3])
    cf = [cv.closed_form(p["A"][0], p["B"][0], p["Q"][0], np.diag(r), p["Qf"][0], N, x0=p["x0"][i],
                         c=p["c"][0], gH=p["gH"][i], gF=p["gF"][i], gf=p["gf"][i]) for i in range(B)]
    ref = {k: np.stack([c[k] for c in cf]) for k in OUTS}
    sh = {k: t[k][0].clone().requires_grad_(True) for k in ("A", "B", "Q", "Qf", "c")}
    x0 = t["x0"].clone().requires_grad_(True)
    Rv = _t(r, dev).requires_grad_(True)
    H, F, f = ag.condense_diff(sh["A"], sh["B"], sh["Q"], Rv, sh["Qf"], N, x0, sh["c"])
    cd = batched.condense(sh["A"].detach(), sh["B"].detach(), sh["Q"].detach(), torch.diag(Rv.detach()),
                          sh["Qf"].detach(), N, x0=x0.detach(), c=sh["c"].detach(),
                          outputs=("H", "F", "f"))
    assert _bits(H.detach(), cd["H"]) and _bits(F.detach(), cd["F"]) and _bits(f.detach(), cd["f"])
    L = (t["gH"] * H).sum() + (t["gF"] * F).sum() + (t["gf"] * f).sum()
    names = ("A", "B", "Q", "Qf", "c")
    got = dict(zip(names + ("x0", "R"),
                   torch.autograd.grad(L, [sh[k] for k in names] + [x0, Rv])))
    for k in names:
        assert got[k].shape == sh[k].shape, k
        assert cv.rel_err(_np(got[k]), ref[GNAME[k]].sum(0)) <= TOL_F64, k
    assert cv.rel_err(_np(got["x0"]), ref["gx0"]) <= TOL_F64
    assert got["R"].shape == (nu,)
    assert cv.rel_err(_np(got["R"]), np.diagonal(ref["gR"].sum(0))) <= TOL_F64
    # a scalar R
    Rs = torch.tensor(0.9, dtype=F64, device=dev, requires_grad=True)
    H, = ag.condense_diff(sh["A"], sh["B"], sh["Q"], Rs, sh["Qf"], N, outputs=("H",))
    gRs, = torch.autograd.grad((t["gH"][0] * H[0]).sum(), [Rs])
    assert gRs.shape == () and cv.rel_err(_np(gRs), np.trace(ref["gR"][0])) <= TOL_F64


# -------------------------------------------------------- mpc_box_model_diff
def test_mpc_box_model_diff(dev):
    """z and status are those of batched.mpc_box; the weight, x0 and bound
    gradients those of mpc_box_diff; the A, B and c gradients the box adjoint's
    closed form (d, d z') carried through the closed form of condensing."""
    p = vc.random_batch()
    nx, nu, N, n, b = p["nx"], p["nu"], p["N"], p["n"], vc.COUNT
    rng = np.random.default_rng(5)
    c_np = 0.1 * rng.standard_normal((N, nx))
    t = {k: _t(p[k], dev) for k in ("A", "B", "Q", "R", "Qf", "x0", "lb", "ub", "g")}
    t["c"] = _t(c_np, dev)
    names = ("A", "B", "Q", "R", "Qf", "x0", "lb", "ub", "c")
    a = {k: t[k].clone().requires_grad_(True) for k in names}
    z, status = ag.mpc_box_model_diff(a["A"], a["B"], a["Q"], a["R"], a["Qf"], N, a["x0"], a["lb"],
                                      a["ub"], a["c"])
    z0, s0 = batched.mpc_box(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], t["lb"], t["ub"],
                             t["c"])
    assert _bits(z.detach(), z0) and torch.equal(status, s0) and not status.requires_grad
    assert (batched.status_code(status) == 0).all()
    got = dict(zip(names, torch.autograd.grad((t["g"] * z).sum(), [a[k] for k in names])))
    old = ("Q", "R", "Qf", "x0", "lb", "ub")
    e = {k: t[k].clone().requires_grad_(True) for k in old}
    z1, _ = ag.mpc_box_diff(t["A"], t["B"], e["Q"], e["R"], e["Qf"], N, e["x0"], e["lb"], e["ub"],
                            t["c"])
    want = dict(zip(old, torch.autograd.grad((t["g"] * z1).sum(), [e[k] for k in old])))
    worst = 0.0
    for k in old:
        assert got[k].shape == want[k].shape, k
        worst = max(worst, cv.rel_err(_np(got[k]), _np(want[k])))
    print(f"mpc_box_model_diff against mpc_box_diff: {worst:.3e}")
    assert worst <= TOL_F64, worst
    zn = _np(z)
    on = (zn == p["lb"]) | (zn == p["ub"])
    assert on.any() and (~on).any()
    H = oc.condense(p["A"], p["B"], p["Q"], p["R"], p["Qf"], N)["H"]
    ref = dict(gA=0.0, gB=0.0, gc=0.0)
    for i in range(b):
        bx = vc.closed_form(H, zn[i], p["lb"][i], p["ub"][i], p["g"][i])
        cf = cv.closed_form(p["A"], p["B"], p["Q"], p["R"], p["Qf"], N, x0=p["x0"][i], c=c_np,
                            gH=bx["gH"], gf=bx["d"])
        for k in ref:
            ref[k] = ref[k] + cf[k]
    worst = max(cv.rel_err(_np(got[k]), ref[GNAME[k]]) for k in ("A", "B", "c"))
    print(f"mpc_box_model_diff A, B, c against the composed closed forms: {worst:.3e}")
    assert worst <= TOL_F64, worst
    assert (got["A"] != 0).any() and (got["c"] != 0).any()
    # the functions that refuse model gradients still do
    with pytest.raises(NotImplementedError, match="A, B"):
        ag.mpc_box_diff(a["A"], t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], -1.0, 1.0)
    with pytest.raises(NotImplementedError):
        ag.mpc_box_model_diff(a["A"], t["B"], t["Q"], t["R"], t["Qf"], 17, t["x0"], -1.0, 1.0)


# --------------------------------------------------- mpc_box_loop_model_diff
def _fhc(dev):
    p = lc.fhc_episode()
    t = {k: _t(p[k], dev) for k in ("A", "B", "Q", "R", "Qf", "x0", "lb", "ub")}
    t["c"] = [_t(c, dev) for c in p["c"]]
    return p, t


def _loss(t, xs, us, zs):
    cx, cu, cz = t["c"]
    return (cx * xs).sum() + (cu * us).sum() + (cz * zs).sum()


def test_mpc_box_loop_model_diff(dev):
    """The FHC episode of _box_loop_vjp_cases (margin 1.4e-2, asserted in
    tests/test_box_loop_vjp_host.py).  Values: batched.mpc_box_loop bit for bit.
    A and B with plant=None: the loop's closed form (gH, gF, gA, gB) with gH, gF
    carried through the closed form of condensing, summed; with plant=(Ap, Bp)
    the two parts separately.  One directional central difference (h = 1e-6) of
    the device loop's loss in A and in B, relative to 1 + |value|: measured
    2.4e-10 and 2.9e-10, bound 1e-4 (a wrong formula shows as O(1))."""
    p, t = _fhc(dev)
    N, steps, nb = lc.FHC_N, lc.FHC_T, lc.FHC_B
    o = batched.mpc_box_loop(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], t["lb"], t["ub"],
                             steps, plans=True)
    names = ("A", "B", "Q", "R", "Qf")
    a = {k: t[k].clone().requires_grad_(True) for k in names}
    xs, us, zs, status = ag.mpc_box_loop_model_diff(a["A"], a["B"], a["Q"], a["R"], a["Qf"], N,
                                                    t["x0"], t["lb"], t["ub"], steps=steps)
    for k, v in (("xs", xs), ("us", us), ("zs", zs)):
        assert _bits(v.detach(), o[k]), k
    assert torch.equal(status, o["status"]) and not status.requires_grad
    assert (batched.status_code(status) == 0).all()
    got = dict(zip(names, torch.autograd.grad(_loss(t, xs, us, zs), [a[k] for k in names])))
    xn, zn = _np(xs), _np(zs)
    cx, cu, cz = p["c"]
    cd = p["cd"]
    plant = dict(gA=0.0, gB=0.0)
    model = dict(gA=0.0, gB=0.0, gQ=0.0, gR=0.0, gQf=0.0)
    for i in range(nb):
        lp = lc.closed_form(p["A"], p["B"], cd["H"], cd["F"], p["lb"], p["ub"], xn[:, i], zn[:, i],
                            cx[:, i], cu[:, i], cz[:, i])
        cf = cv.closed_form(p["A"], p["B"], p["Q"], p["R"], p["Qf"], N, gH=lp["gH"], gF=lp["gF"])
        plant = {k: plant[k] + lp[k] for k in plant}
        model = {k: model[k] + cf[k] for k in model}
    worst = max(cv.rel_err(_np(got["A"]), plant["gA"] + model["gA"]),
                cv.rel_err(_np(got["B"]), plant["gB"] + model["gB"]),
                cv.rel_err(_np(got["Q"]), model["gQ"]), cv.rel_err(_np(got["R"]), model["gR"]),
                cv.rel_err(_np(got["Qf"]), model["gQf"]))
    print(f"mpc_box_loop_model_diff, plant=None: {worst:.3e}")
    assert worst <= TOL_EPISODE, worst

    # a simulated plant of its own: the two parts come out separately
    Ap, Bp = t["A"].clone().requires_grad_(True), t["B"].clone().requires_grad_(True)
    xs2, us2, zs2, st2 = ag.mpc_box_loop_model_diff(a["A"], a["B"], t["Q"], t["R"], t["Qf"], N,
                                                    t["x0"], t["lb"], t["ub"], steps=steps,
                                                    plant=(Ap, Bp))
    assert _bits(xs2.detach(), o["xs"]) and _bits(zs2.detach(), o["zs"])
    gAm, gBm, gAp, gBp = torch.autograd.grad(_loss(t, xs2, us2, zs2), [a["A"], a["B"], Ap, Bp])
    worst = max(cv.rel_err(_np(gAm), model["gA"]), cv.rel_err(_np(gBm), model["gB"]),
                cv.rel_err(_np(gAp), plant["gA"]), cv.rel_err(_np(gBp), plant["gB"]))
    print(f"mpc_box_loop_model_diff, plant=(Ap, Bp): {worst:.3e}")
    assert worst <= TOL_EPISODE, worst

    # the device loop itself, moved along one direction in A and one in B
    rng = np.random.default_rng(21)
    h = 1e-6

    def loop_loss(A_, B_):
        r = batched.mpc_box_loop(A_, B_, t["Q"], t["R"], t["Qf"], N, t["x0"], t["lb"], t["ub"],
                                 steps, plans=True)
        assert (batched.status_code(r["status"]) == 0).all()
        return float(_loss(t, r["xs"], r["us"], r["zs"]))

    for k in ("A", "B"):
        D = _t(rng.standard_normal(p[k].shape), dev)
        up = {"A": t["A"], "B": t["B"], k: t[k] + h * D}
        dn = {"A": t["A"], "B": t["B"], k: t[k] - h * D}
        fd = (loop_loss(up["A"], up["B"]) - loop_loss(dn["A"], dn["B"])) / (2 * h)
        an = float((got[k] * D).sum())
        err = abs(fd - an) / (1 + abs(an))
        print(f"mpc_box_loop_model_diff: central difference in {k}: fd {fd:.9e}, analytic "
              f"{an:.9e}, relative {err:.3e}")
        assert err <= 1e-4, (k, fd, an)


def test_mpc_box_loop_model_diff_references_and_errors(dev):
    """u_ref and w: values of batched.mpc_box_loop bit for bit, gradients
    reach them; x_ref raises; the size limits raise; mpc_box_loop_diff still
    refuses A."""
    p, t = _fhc(dev)
    N, steps = lc.FHC_N, lc.FHC_T
    rng = np.random.default_rng(12)
    u_ref = _t(0.2 * rng.standard_normal((steps + N, 1)), dev).requires_grad_(True)
    w = _t(0.02 * rng.standard_normal((steps, lc.FHC_B, 2)), dev).requires_grad_(True)
    A = t["A"].clone().requires_grad_(True)
    R = t["R"].clone().requires_grad_(True)
    o = batched.mpc_box_loop(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], -1.0, 1.0, steps,
                             plans=True, u_ref=u_ref.detach(), w=w.detach())
    xs, us, zs, status = ag.mpc_box_loop_model_diff(A, t["B"], t["Q"], R, t["Qf"], N, t["x0"], -1.0,
                                                    1.0, steps=steps, u_ref=u_ref, w=w)
    for k, v in (("xs", xs), ("us", us), ("zs", zs)):
        assert _bits(v.detach(), o[k]), k
    assert torch.equal(status, o["status"])
    gA, gR, gu, gw = torch.autograd.grad(_loss(t, xs, us, zs), (A, R, u_ref, w))
    assert torch.isfinite(gA).all() and (gA != 0).any() and torch.isfinite(gR).all()
    assert (gu != 0).any() and (gw != 0).any()
    x_ref = _t(0.3 * rng.standard_normal((steps + N + 1, 2)), dev)
    with pytest.raises(NotImplementedError, match="x_ref"):
        ag.mpc_box_loop_model_diff(A, t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], -1.0, 1.0,
                                   steps=steps, x_ref=x_ref)
    with pytest.raises(NotImplementedError, match="N \\* nu"):
        ag.mpc_box_loop_model_diff(A, t["B"], t["Q"], t["R"], t["Qf"], 33, t["x0"], -1.0, 1.0,
                                   steps=steps)
    with pytest.raises(NotImplementedError):
        ag.mpc_box_loop_diff(A, t["B"], t["Q"], t["R"], t["Qf"], N, t["x0"], -1.0, 1.0, steps=steps)
    import model_predictive_control_amd as pkg
    assert pkg.mpc_box_model_diff is ag.mpc_box_model_diff
    assert pkg.mpc_box_loop_model_diff is ag.mpc_box_loop_model_diff
    H1, = pkg.condense_diff(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, outputs=("H",))
    H2, = ag.condense_diff(t["A"], t["B"], t["Q"], t["R"], t["Qf"], N, outputs=("H",))
    assert _bits(H1, H2)
