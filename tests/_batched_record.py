"""Recorder of what ``batched`` hands to libmpcqp, for the characterisation test
tests/test_batched_marshal_host.py.

Four names of the ``batched`` module are replaced while a case runs: ``_lib``
by a recorder (every attribute is a function that notes ``(entry, args)`` and
returns 0, or a fixed byte count for the ``*workspace`` queries), ``_stream``
by ``lambda: 0``, ``_workspace`` by a CPU uint8 allocation (or the caller's
``ws``) and ``_dev`` by the same conversion without the device requirement.  The
wrappers then run on CPU tensors; nothing is launched.

A recorded call is the entry's name and its arguments: numbers as they are,
the bicycle parameter arrays as lists, and every pointer as None, "empty" (a
tensor without elements), the label of the case's input it points into,
["new", shape, dtype] for a tensor the wrapper allocated (torch.empty /
torch.zeros) or ["conv", shape, dtype] for one it made from an input.  The
result is recorded by structure (shapes, dtypes, which tensors are the
caller's own objects), a failure by the exception's class and text.

``PYTHONPATH=. python tests/_batched_record.py OUT.json COMMIT`` writes the
golden file; it is run in a checkout of the parent commit (with this file
copied in), never on the tree under test.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import json
import math
import sys
import types
import warnings

import torch

from model_predictive_control_amd import _native as nat
from model_predictive_control_amd import batched as bt

WS_BYTES = 4096
F64, F32, I32 = torch.float64, torch.float32, torch.int32

_ORIG = {k: getattr(bt, k) for k in ("_lib", "_stream", "_workspace", "_dev")}


def _fake_dev(x, dtype, device):
    if x is None:
        return None
    return torch.as_tensor(x, dtype=dtype, device=device).contiguous()


def _fake_workspace(nbytes, dev, ws=None):
    if nbytes <= 0:
        return None
    if ws is not None:
        return ws
    return torch.empty((int(nbytes),), dtype=torch.uint8)


class Ctx:
    """One case: its labelled inputs, the tensors allocated while it runs and
    the calls it records."""

    def __init__(self):
        self.labels, self.objs, self.new, self.calls = {}, [], {}, []

    def inp(self, label, t):
        if isinstance(t, torch.Tensor):
            self.labels.setdefault(t.data_ptr(), label)
            self.objs.append((label, t))
        return t

    def label_of(self, t):
        for label, o in self.objs:
            if o is t:
                return label
        return None

    # ---- the recorder library
    def _pointer(self, p):
        if p is None:
            return None
        if p == 0:
            return "empty"
        if p in self.labels:
            return self.labels[p]
        if p in self.new:
            t = self.new[p]
            return ["new", list(t.shape), str(t.dtype)]
        with warnings.catch_warnings():     # isinstance on every live object trips deprecations
            warnings.simplefilter("ignore")
            found = [o for o in gc.get_objects() if isinstance(o, torch.Tensor) and o.numel()
                     and o.data_ptr() == p]
        if not found:
            return ["unknown"]
        t = min(found, key=lambda o: (-o.numel(), str(tuple(o.shape))))
        return ["conv", list(t.shape), str(t.dtype)]

    def _record(self, name, args):
        kinds = nat.SIGNATURES[name][1] if name in nat.SIGNATURES else [None] * len(args)
        rec = []
        for a, k in zip(args, list(kinds) + [None] * (len(args) - len(kinds))):
            if isinstance(a, ctypes.Array):
                rec.append(list(a))
            elif k is ctypes.c_void_p or a is None:
                rec.append(self._pointer(a))
            elif isinstance(a, bool):
                rec.append(int(a))
            else:
                rec.append(a)
        self.calls.append([name, rec])
        return WS_BYTES if name.endswith("workspace") else 0

    def __getattr__(self, name):
        if not name.startswith("mpcqp_"):
            raise AttributeError(name)
        return lambda *args: self._record(name, args)


@contextlib.contextmanager
def patched(ctx):
    """The four seams of ``batched`` replaced, and torch.empty / torch.zeros
    noting what they allocate."""
    real = {"empty": torch.empty, "zeros": torch.zeros}

    def noting(fn):
        def alloc(*a, **k):
            t = fn(*a, **k)
            if t.numel():
                ctx.new[t.data_ptr()] = t
            return t
        return alloc

    bt._lib, bt._stream = (lambda: ctx), (lambda: 0)
    bt._workspace, bt._dev = _fake_workspace, _fake_dev
    torch.empty, torch.zeros = noting(real["empty"]), noting(real["zeros"])
    try:
        yield
    finally:
        torch.empty, torch.zeros = real["empty"], real["zeros"]
        for k, v in _ORIG.items():
            setattr(bt, k, v)


def _structure(r, ctx, values):
    if isinstance(r, torch.Tensor):
        d = {"shape": list(r.shape), "dtype": str(r.dtype), "is": ctx.label_of(r)}
        if values:
            d["values"] = [round(float(v), 9) for v in r.reshape(-1).tolist()]
        return d
    if isinstance(r, dict):
        return {"dict": {k: _structure(r[k], ctx, values) for k in sorted(r)}}
    if isinstance(r, (tuple, list)):
        return {type(r).__name__: [_structure(v, ctx, values) for v in r]}
    if isinstance(r, bt.PolyQP):
        return {"PolyQP": [r.n, r.m, r.nx, r.nbox, r.mt]}
    if r is None or isinstance(r, (int, float, str)):
        return r
    return repr(r)


def run_case(fn):
    ctx = Ctx()
    values = getattr(fn, "values", False)
    rec = {}
    with patched(ctx):
        try:
            rec["ret"] = _structure(fn(ctx), ctx, values)
        except Exception as e:  # noqa: BLE001 -- the class and text are the record
            rec["error"] = [type(e).__name__, str(e)]
    rec["calls"] = ctx.calls
    return json.loads(json.dumps(rec))


def record_all():
    return {name: run_case(fn) for name, fn in CASES.items()}


# ------------------------------------------------------------------ the cases
CASES: dict = {}


def case(fn=None, *, values=False):
    def reg(f):
        name = f.__name__
        assert name not in CASES, name
        f.values = values
        CASES[name] = f
        return f
    return reg(fn) if fn is not None else reg


def T(*shape, dt=F64, k=1.0):
    """A deterministic tensor of this shape."""
    n = math.prod(shape)
    return (torch.arange(n, dtype=F64).reshape(shape) * 0.01 * k + k).to(dt)


def plant(c, nx=2, nu=1, N=3, b=2, per="", tv=False, dt=F64, only=None):
    """Labelled A, B, Q, R, Qf; the names in ``per`` carry a batch dimension."""
    base = {"A": (N, nx, nx) if tv else (nx, nx), "B": (N, nx, nu) if tv else (nx, nu),
            "Q": (nx, nx), "R": (nu, nu), "Qf": (nx, nx)}
    return [c.inp(k, T(*(((b,) if k in per.split() else ()) + base[k]), dt=dt, k=i + 1.0))
            for i, k in enumerate(base) if only is None or k in only]


def bounds(c, form, n, b, names=("lb", "ub"), dt=F64):
    """A lower/upper pair in one of the forms a bound may take."""
    def one(name, f, k):
        if f == "none":
            return None
        if f == "scalar":
            return float(k)
        if f == "int":
            return int(k)
        if f == "0d":
            return c.inp(name, torch.tensor(float(k), dtype=dt))
        if f == "shared":
            return c.inp(name, T(n, dt=dt, k=k))
        if f == "per":
            return c.inp(name, T(b, n, dt=dt, k=k))
        if f == "3d":
            return c.inp(name, T(1, b, n, dt=dt, k=k))
        raise KeyError(f)
    lo, hi = form if isinstance(form, tuple) else (form, form)
    return one(names[0], lo, -1), one(names[1], hi, 1)


BOUND_FORMS = ("none", "scalar", "0d", "shared", "per", ("shared", "per"), ("per", "none"),
               ("int", "shared"))


def _form_name(f):
    return "_".join(f) if isinstance(f, tuple) else f


# ---- condense
def _condense_case(name, per="", tv=False, x0=None, cc=None, dt=F64, **kw):
    def f(c):
        nx, nu, N, b = 2, 1, 3, 2
        ops = plant(c, nx, nu, N, b, per, tv, dt)
        x = None if x0 is None else c.inp("x0", T(*((b, nx) if x0 == "per" else (nx,)), dt=dt))
        cv = None if cc is None else c.inp("c", T(*((b, N, nx) if cc == "per" else (N, nx)), dt=dt))
        k = dict(kw)
        if k.get("out") == "given":
            k["out"] = {"H": c.inp("out.H", torch.empty((b if per or x0 == "per" else 1, 6), dtype=dt)),
                        "f": c.inp("out.f", torch.empty((b if per or x0 == "per" else 1, 3), dtype=dt))}
        return bt.condense(*ops, N, x, cv, tv=tv, **k)
    f.__name__ = "condense_" + name
    case(f)


_condense_case("shared")
_condense_case("per_AB", per="A B", x0="per", cc="per")
_condense_case("per_weights", per="Q R Qf", x0="shared", cc="shared")
_condense_case("per_x0_only", x0="per")
_condense_case("tv_shared", tv=True)
_condense_case("tv_per", per="A B", tv=True, x0="per")
_condense_case("all_outputs", outputs=("H", "F", "f", "Gam", "Phi", "xbar"), x0="shared")
_condense_case("gam_packed", outputs=("Gam",), gam_packed=True)
_condense_case("out_given", x0="per", out="given")
_condense_case("f32", dt=F32, x0="per")


@case
def condense_r_vector(c):
    A, B, Q, R, Qf = plant(c)
    return bt.condense(A, B, Q, c.inp("R1", T(1)), Qf, 3)


@case
def condense_noncontiguous(c):
    A, B, Q, R, Qf = plant(c, per="A")
    return bt.condense(c.inp("At", A.transpose(1, 2)), B, Q, R, Qf, 3)


@case
def condense_err_r_vector(c):
    A, B, Q, R, Qf = plant(c, nu=2)
    return bt.condense(A, B, Q, T(2), Qf, 3)


@case
def condense_err_dims(c):
    A, B, Q, R, Qf = plant(c)
    return bt.condense(T(1, 3, 2, 2), B, Q, R, Qf, 3)


@case
def condense_err_batch(c):
    A, B, Q, R, Qf = plant(c, per="A")
    return bt.condense(A, T(3, 2, 1), Q, R, Qf, 3)


@case
def condense_err_r_then_dims(c):
    """R malformed and A malformed: R's message wins."""
    A, B, Q, R, Qf = plant(c)
    return bt.condense(T(1, 3, 2, 2), B, Q, T(2), Qf, 3)


@case
def condense_err_dims_then_batch(c):
    """Q has too many dimensions and A, B disagree on the batch: Q's message wins."""
    A, B, Q, R, Qf = plant(c, per="A")
    return bt.condense(A, T(3, 2, 1), T(1, 2, 2, 2), R, Qf, 3)


# ---- mpc_box
def _mpc_box_case(name, per="", tv=False, form="none", x0="per", cc=None, out=False, dt=F64,
                  **kw):
    def f(c):
        nx, nu, N, b = 2, 1, 3, 2
        ops = plant(c, nx, nu, N, b, per, tv, dt)
        x = c.inp("x0", T(*((b, nx) if x0 == "per" else (nx,)), dt=dt))
        cv = None if cc is None else c.inp("c", T(*((b, N, nx) if cc == "per" else (N, nx)), dt=dt))
        lb, ub = bounds(c, form, N * nu, b, dt=dt)
        o = None
        if out:
            o = (c.inp("out.z", torch.empty((b, N * nu), dtype=dt)),
                 c.inp("out.status", torch.empty((b,), dtype=I32)))
        return bt.mpc_box(*ops, N, x, lb, ub, cv, tv=tv, out=o, **kw)
    f.__name__ = "mpc_box_" + name
    case(f)


for _f in BOUND_FORMS:
    _mpc_box_case("bounds_" + _form_name(_f), form=_f)
_mpc_box_case("per_AB", per="A B", form="scalar", cc="per")
_mpc_box_case("per_weights", per="Q R Qf", x0="shared", cc="shared")
_mpc_box_case("shared_all", x0="shared", form=("shared", "shared"))
_mpc_box_case("tv_shared", tv=True, form="scalar")
_mpc_box_case("tv_per", per="A B", tv=True)
_mpc_box_case("out_given", out=True, form="scalar", max_iter=7, tol=1e-9)
_mpc_box_case("f32", dt=F32, form="scalar")


@case
def mpc_box_err_bound_dims(c):
    ops = plant(c)
    return bt.mpc_box(*ops, 3, T(2, 2), T(1, 2, 3), None)


@case
def mpc_box_err_bound_batch(c):
    ops = plant(c)
    return bt.mpc_box(*ops, 3, T(2, 2), T(3, 3), None)


@case
def mpc_box_err_r_then_bound(c):
    """R malformed and a bound with too many dimensions: R's message wins."""
    A, B, Q, R, Qf = plant(c, nu=2)
    return bt.mpc_box(A, B, Q, T(2), Qf, 3, T(2, 2), T(1, 2, 6), None)


@case
def mpc_box_err_dims_then_bound(c):
    """x0 and lb both have too many dimensions: x0's message wins."""
    ops = plant(c)
    return bt.mpc_box(*ops, 3, T(1, 2, 2), T(1, 2, 3), None)


@case
def mpc_box_err_bound_then_batch(c):
    """ub has too many dimensions and A, x0 disagree on the batch: ub's message wins."""
    ops = plant(c, per="A")
    return bt.mpc_box(*ops, 3, T(3, 2), None, T(1, 2, 3))


# ---- mpc_qp / mpc_ipm
def _sbounds(c, form, nx, N, b):
    def one(name, f, k):
        shp = {"none": None, "stage": (nx,), "shared": (N * nx,), "per": (b, N * nx),
               "bad": (N * nx + 1,), "3d": (1, b, N * nx)}[f]
        return None if shp is None else c.inp(name, T(*shp, k=k))
    lo, hi = form if isinstance(form, tuple) else (form, form)
    return one("xlo", lo, -2), one("xhi", hi, 2)


def _mpc_qp_case(name, per="", tv=False, sform="shared", form="scalar", x0="per", out=0, ws=False,
                 fn="mpc_qp", nx=2, N=3, **kw):
    def f(c):
        nu, b = 1, 2
        ops = plant(c, nx, nu, N, b, per, tv)
        x = c.inp("x0", T(*((b, nx) if x0 == "per" else (nx,))))
        xlo, xhi = _sbounds(c, sform, nx, N, b)
        lb, ub = bounds(c, form, N * nu, b)
        k = dict(kw)
        if out and fn == "mpc_qp":
            o = [c.inp("out.z", torch.empty((b, N * nu), dtype=F64)),
                 c.inp("out.y", torch.empty((b, N * nx), dtype=F64)),
                 c.inp("out.status", torch.empty((b,), dtype=I32))]
            if out == 4:
                o.append(c.inp("out.X", torch.empty((b, N, nx), dtype=F64)))
            k["out"] = tuple(o)
        elif out:
            k["out"] = {"z": c.inp("out.z", torch.empty((b, N * nu), dtype=F64)),
                        "status": c.inp("out.status", torch.empty((b,), dtype=I32))}
        if ws:
            k["ws"] = c.inp("ws", torch.empty((2 * WS_BYTES,), dtype=torch.uint8))
        return getattr(bt, fn)(*ops, N, x, xlo, xhi, lb, ub, None, tv=tv, **k)
    f.__name__ = fn + "_" + name
    case(f)


for _f in ("none", "stage", "shared", "per", ("shared", "none"), ("none", "per")):
    _mpc_qp_case("sbounds_" + _form_name(_f), sform=_f)
for _f in BOUND_FORMS:
    _mpc_qp_case("bounds_" + _form_name(_f), form=_f)
_mpc_qp_case("stage_is_whole", sform="stage", N=1)
_mpc_qp_case("per_AB", per="A B")
_mpc_qp_case("per_weights", per="Q R Qf", x0="shared")
_mpc_qp_case("tv_shared", tv=True)
_mpc_qp_case("tv_per", per="A B", tv=True, ipm=True)
_mpc_qp_case("states", states=True)
_mpc_qp_case("out3", out=3)
_mpc_qp_case("out4_states", out=4, states=True, max_iter=5, tol=1e-8)
_mpc_qp_case("out_ws", out=3, ws=True)
_mpc_qp_case("err_sbound_size", sform="bad")
_mpc_qp_case("err_sbound_dims", sform="3d")
_mpc_qp_case("err_sbound_mixed", sform=("shared", "per"))
_mpc_qp_case("err_sbound_then_bound", sform="bad", form="3d")
_mpc_qp_case("err_bound_dims", form="3d")

_mpc_qp_case("plain", fn="mpc_ipm")
_mpc_qp_case("per_tv", fn="mpc_ipm", per="A B", tv=True, sform="per", form="per")
_mpc_qp_case("out_ws", fn="mpc_ipm", out=1, ws=True, strict=True, max_iter=9, tol=1e-7)
_mpc_qp_case("err_sbound_mixed", fn="mpc_ipm", sform=("per", "shared"))


@case
def mpc_qp_err_r_then_sbound(c):
    """R malformed and a state bound of the wrong size: R's message wins."""
    A, B, Q, R, Qf = plant(c, nu=2)
    return bt.mpc_qp(A, B, Q, T(2), Qf, 3, T(2, 2), T(7), None)


@case
def mpc_qp_err_dims_then_sbound(c):
    """B has too many dimensions and a state bound the wrong size: B's message wins."""
    A, B, Q, R, Qf = plant(c)
    return bt.mpc_qp(A, T(1, 2, 2, 1), Q, R, Qf, 3, T(2, 2), T(7), None)


@case
def mpc_qp_err_batch(c):
    ops = plant(c, per="A")
    return bt.mpc_qp(*ops, 3, T(2, 2), T(3, 6), None)


@case
def mpc_ipm_extras(c):
    ops = plant(c)
    b, N, nx, nu = 2, 3, 2, 1
    return bt.mpc_ipm(*ops, N, c.inp("x0", T(b, nx)), None, None, -1.0, 1.0,
                      U0=c.inp("U0", T(b, N, nu)), H2=c.inp("H2", T(b, N, 3, 3)),
                      q2=c.inp("q2", T(b, N, 3)), skip=c.inp("skip", torch.zeros(b, dtype=I32)),
                      skip_mask=3)


@case
def mpc_ipm_u0_flat(c):
    ops = plant(c)
    return bt.mpc_ipm(*ops, 3, c.inp("x0", T(2, 2)), U0=c.inp("U0", T(2, 3)), skip_mask=5)


@case
def mpc_ipm_err_skip(c):
    ops = plant(c)
    return bt.mpc_ipm(*ops, 3, T(2, 2), skip=torch.zeros(3, dtype=I32), skip_mask=1)


@case
def mpc_ipm_err_skip_dtype(c):
    ops = plant(c)
    return bt.mpc_ipm(*ops, 3, T(2, 2), skip=torch.zeros(2, dtype=torch.int64), skip_mask=1)


# ---- mpc_box_loop
def _cd(c, b, n, nx, gam=False, N=3):
    cd = {"H": c.inp("cd.H", T(b, n * (n + 1) // 2)), "F": c.inp("cd.F", T(b, n, nx, k=2))}
    if gam:
        cd["Gam"] = c.inp("cd.Gam", T(b, N * nx, n, k=3))
    return cd


def _box_loop_case(name, per="", cdb=1, form="scalar", g=None, w=False, ref=None, out=False,
                   b=2, steps=4, use_cd=True, gam=False, **kw):
    def f(c):
        nx, nu, N = 2, 1, 3
        n = N * nu
        ops = plant(c, nx, nu, N, b, per)
        x = c.inp("x0", T(b, nx))
        lb, ub = bounds(c, form, n, b)
        k = dict(kw)
        if use_cd:
            k["condensed"] = _cd(c, cdb, n, nx, gam)
        if g is not None:
            k["g"] = c.inp("g", T(*{"shared": (steps, n), "per": (steps, b, n),
                                     "bad": (steps, n + 1)}[g]))
        if w:
            k["w"] = c.inp("w", T(*((steps, b, nx) if w is True else w)))
        if ref == "x":
            k["x_ref"] = c.inp("x_ref", T(nx))
        if ref == "xu":
            k["x_ref"] = c.inp("x_ref", T(steps + N + 1, nx))
            k["u_ref"] = c.inp("u_ref", T(b, steps + N, nu))
        if out:
            k["out"] = {"xs": c.inp("out.xs", torch.empty((steps + 1, b, nx), dtype=F64)),
                        "status": c.inp("out.status", torch.empty((steps, b), dtype=I32))}
        return bt.mpc_box_loop(*ops, N, x, lb, ub, steps, **k)
    f.__name__ = "mpc_box_loop_" + name
    case(f)


_box_loop_case("plain")
_box_loop_case("plain_per_plant", per="A B", cdb=2, form="per")
_box_loop_case("condense_inside", use_cd=False)
_box_loop_case("condense_inside_per", use_cd=False, per="A B")
_box_loop_case("plans_out", plans=True, out=True, max_iter=3, tol=1e-6)
_box_loop_case("g_shared", g="shared")
_box_loop_case("g_per", g="per", plans=True)
_box_loop_case("w", w=True)
_box_loop_case("cold", cold=True)
_box_loop_case("x_ref", ref="x", gam=True)
_box_loop_case("x_ref_no_gam", ref="x")
_box_loop_case("xu_ref_condense_inside", ref="xu", use_cd=False)
_box_loop_case("leading_one_batch_one", b=1)
_box_loop_case("leading_one", cdb=1, b=3)
for _f in BOUND_FORMS:
    _box_loop_case("bounds_" + _form_name(_f), form=_f)
_box_loop_case("err_g_and_ref", g="shared", ref="x")
_box_loop_case("err_g_shape", g="bad")
_box_loop_case("err_w_shape", w=(4, 2, 3))


@case
def mpc_box_loop_shared_cd(c):
    """H and F without a batch dimension."""
    ops = plant(c)
    cd = {"H": c.inp("cd.H", T(6)), "F": c.inp("cd.F", T(3, 2))}
    return bt.mpc_box_loop(*ops, 3, c.inp("x0", T(2, 2)), -1.0, 1.0, 2, condensed=cd)


@case
def mpc_box_loop_err_x0(c):
    ops = plant(c)
    return bt.mpc_box_loop(*ops, 3, T(2), -1.0, 1.0, 2)


@case
def mpc_box_loop_err_x0_then_g(c):
    ops = plant(c)
    return bt.mpc_box_loop(*ops, 3, T(2, 3), -1.0, 1.0, 2, g=T(2, 3), x_ref=T(2))


# ---- solve_box / solve_box_vjp
def _solve_box_case(name, hper=True, fper=True, form="scalar", out=False, ws=False, dt=F64,
                    n=4, fn="solve_box", **kw):
    def f(c):
        b = 3
        H = c.inp("H", T(*((b,) if hper else ()) + (n * (n + 1) // 2,), dt=dt))
        fv = c.inp("f", T(*((b,) if fper else ()) + (n,), dt=dt, k=2))
        lb, ub = bounds(c, form, n, b, dt=dt)
        k = dict(kw)
        if out:
            k["out"] = (c.inp("out.z", torch.empty((b, n), dtype=dt)),
                        c.inp("out.status", torch.empty((b,), dtype=I32)))
        if ws:
            k["ws"] = c.inp("ws", torch.empty((WS_BYTES,), dtype=torch.uint8))
        return bt.solve_box(H, fv, lb, ub, **k)
    f.__name__ = "solve_box_" + name
    case(f)


for _f in BOUND_FORMS:
    _solve_box_case("bounds_" + _form_name(_f), form=_f)
_solve_box_case("shared_H", hper=False)
_solve_box_case("shared_f", fper=False)
_solve_box_case("all_shared", hper=False, fper=False, form="shared")
_solve_box_case("out_ws", out=True, ws=True, max_iter=11, tol=1e-10)
_solve_box_case("no_presweep", presweep=False)
_solve_box_case("f32", dt=F32)
_solve_box_case("err_dtype", dt=torch.float16)
_solve_box_case("err_bound_dims", form="3d")


@case
def solve_box_err_packed(c):
    return bt.solve_box(T(3, 9), T(3, 4))


@case
def solve_box_err_dims(c):
    return bt.solve_box(T(1, 3, 10), T(3, 4))


@case
def solve_box_err_batch(c):
    return bt.solve_box(T(2, 10), T(3, 4))


@case
def solve_box_err_empty_batch(c):
    return bt.solve_box(T(0, 10), T(0, 4))


@case
def solve_box_err_empty_bound(c):
    return bt.solve_box(T(10), T(4), T(0, 4))


@case
def condense_err_empty_batch(c):
    A, B, Q, R, Qf = plant(c)
    return bt.condense(A, B, Q, R, Qf, 3, T(0, 2))


def _box_vjp_case(name, hper=True, form="per", status=None, b=3, n=4, **kw):
    def f(c):
        H = c.inp("H", T(*((b,) if hper else ()) + (n * (n + 1) // 2,)))
        z, gz = c.inp("z", T(b, n)), c.inp("gz", T(b, n, k=2))
        lb, ub = bounds(c, form, n, b)
        st = None
        if status == "ok":
            st = c.inp("status", torch.zeros(b, dtype=I32))
        elif status == "bad":
            st = torch.zeros(b + 1, dtype=I32)
        elif status == "dtype":
            st = torch.zeros(b, dtype=torch.int64)
        return bt.solve_box_vjp(H, z, lb, ub, gz, status=st, **kw)
    f.__name__ = "solve_box_vjp_" + name
    case(f)


for _f in BOUND_FORMS:
    _box_vjp_case("bounds_" + _form_name(_f), form=_f)
_box_vjp_case("shared_H", hper=False, form="shared")
_box_vjp_case("status_no_gH", status="ok", need_H=False)
_box_vjp_case("err_status", status="bad")
_box_vjp_case("err_status_dtype", status="dtype")
_box_vjp_case("err_bound_dims", form="3d")


@case
def solve_box_vjp_err_gz(c):
    return bt.solve_box_vjp(T(3, 10), T(3, 4), None, None, T(3, 5))


@case
def solve_box_vjp_err_z_dims(c):
    return bt.solve_box_vjp(T(10), T(4), None, None, T(4))


@case
def solve_box_vjp_err_packed(c):
    return bt.solve_box_vjp(T(3, 9), T(3, 4), None, None, T(3, 4))


@case
def solve_box_vjp_err_bound_width(c):
    return bt.solve_box_vjp(T(3, 10), T(3, 4), T(5), None, T(3, 4))


@case
def solve_box_vjp_err_ub_width_and_status(c):
    return bt.solve_box_vjp(T(3, 10), T(3, 4), None, T(3, 5), T(3, 4),
                            status=torch.zeros(2, dtype=I32))


@case
def solve_box_vjp_err_batch(c):
    return bt.solve_box_vjp(T(2, 10), T(3, 4), None, None, T(3, 4))


@case
def solve_box_vjp_err_bound_batch(c):
    return bt.solve_box_vjp(T(3, 10), T(3, 4), T(2, 4), None, T(3, 4))


# ---- mpc_box_loop_vjp
def _loop_vjp_case(name, lead=None, form="scalar", b=3, status=None, ups="all", T_=4,
                   bad=None, **kw):
    """``lead``: None = shared operands without a batch dimension, else the
    leading dimension of H, F, A, B."""
    def f(c):
        nx, nu, N = 2, 1, 3
        n = N * nu
        pre = () if lead is None else (lead,)
        H = c.inp("H", T(*pre, n * (n + 1) // 2))
        F = c.inp("F", T(*pre, n, nx, k=2))
        A = c.inp("A", T(*pre, nx, nx, k=3))
        B = c.inp("B", T(*pre, nx, nu, k=4))
        lb, ub = bounds(c, form, n, b)
        xs = c.inp("xs", T(T_ + 1, b, nx))
        zs = c.inp("zs", T(T_, b, n))
        g = {"gxs": c.inp("gxs", T(T_ + 1, b, nx)), "gus": c.inp("gus", T(T_, b, nu)),
             "gzs": c.inp("gzs", T(T_, b, n))}
        if ups == "none":
            g = dict.fromkeys(g)
        if bad in g:
            g[bad] = T(T_, b, 7)
        st = None
        if status == "ok":
            st = c.inp("status", torch.zeros((T_, b), dtype=I32))
        elif status == "bad":
            st = torch.zeros((b,), dtype=I32)
        if bad == "F":
            F = T(*pre, n, nx + 1)
        if bad == "xs":
            xs = T(T_, b, nx)
        return bt.mpc_box_loop_vjp(H, F, A, B, lb, ub, xs, zs, g["gxs"], g["gus"], g["gzs"],
                                   status=st, **kw)
    f.__name__ = "mpc_box_loop_vjp_" + name
    case(f)


_loop_vjp_case("shared")
_loop_vjp_case("per", lead=3, form="per", status="ok")
_loop_vjp_case("leading_one", lead=1)
_loop_vjp_case("leading_one_batch_one", lead=1, b=1)
_loop_vjp_case("no_upstream_need_some", ups="none", need=("gx0", "gF", "glb"))
for _f in BOUND_FORMS:
    _loop_vjp_case("bounds_" + _form_name(_f), form=_f)
_loop_vjp_case("err_status", status="bad")
_loop_vjp_case("err_need", need=("gx0", "gQ"))
_loop_vjp_case("err_gus", bad="gus")
_loop_vjp_case("err_shapes", bad="F")
_loop_vjp_case("err_xs", bad="xs")
_loop_vjp_case("err_batch", lead=2)
_loop_vjp_case("err_bound_dims", form="3d")
_loop_vjp_case("err_shapes_and_need", bad="F", need=("nope",))


@case
def mpc_box_loop_vjp_err_bound_width(c):
    return bt.mpc_box_loop_vjp(T(6), T(3, 2), T(2, 2), T(2, 1), None, T(4), T(5, 3, 2), T(4, 3, 3))


# ---- polytope QP
def _rows(c, form, m, b, names=("hl", "hu")):
    def one(name, f, k):
        shp = {"none": None, "shared": (m,), "per": (b, m), "per2": (b + 1, m), "wide": (m + 1,),
               "3d": (1, b, m)}[f]
        return None if shp is None else c.inp(name, T(*shp, k=k))
    lo, hi = form if isinstance(form, tuple) else (form, form)
    return one(names[0], lo, -3), one(names[1], hi, 3)


def _poly_out_arg(c, out, b, n, mt):
    if out == "given":
        return (c.inp("out.z", torch.empty((b, n), dtype=F64)),
                c.inp("out.y", torch.empty((b, mt), dtype=F64)),
                c.inp("out.status", torch.empty((b,), dtype=I32)))
    if out == "list":
        return [c.inp("out.z", torch.empty((b, n), dtype=F64)),
                c.inp("out.y", torch.empty((b, mt), dtype=F64)),
                c.inp("out.status", torch.empty((b,), dtype=I32))]
    if out == "pair":
        return (torch.empty((b, n), dtype=F64), torch.empty((b,), dtype=I32))
    if out == "shape":
        return (torch.empty((b, n), dtype=F64), torch.empty((b, mt + 1), dtype=F64),
                torch.empty((b,), dtype=I32))
    if out == "dtype":
        return (torch.empty((b, n), dtype=F64), torch.empty((b, mt), dtype=F64),
                torch.empty((b,), dtype=torch.int64))
    if out == "strided":
        return (torch.empty((n, b), dtype=F64).T, torch.empty((b, mt), dtype=F64),
                torch.empty((b,), dtype=I32))
    return None


def _solve_poly_case(name, fper=True, G=True, rows="shared", box="scalar", out=None, **kw):
    def f(c):
        n, m, b = 3, 2, 2
        H = c.inp("H", T(6))
        fv = c.inp("f", T(*((b, n) if fper else (n,)), k=2))
        Gm = c.inp("G", T(m, n, k=3)) if G else None
        hl, hu = _rows(c, rows, m if G else 0, b)
        lbz, ubz = bounds(c, box, n, b, names=("lbz", "ubz"))
        mt = (m if G else 0) + (n if box != "none" else 0)
        return bt.solve_poly(H, fv, Gm, hl, hu, lbz, ubz, out=_poly_out_arg(c, out, b, n, mt), **kw)
    f.__name__ = "solve_poly_" + name
    case(f)


_solve_poly_case("plain")
_solve_poly_case("shared_f", fper=False)
_solve_poly_case("rows_per", rows="per", box="none")
_solve_poly_case("rows_hl_only", rows=("per", "none"), box="shared")
_solve_poly_case("rows_hu_only", rows=("none", "shared"), box="0d")
_solve_poly_case("no_G", G=False, rows="none", box=("none", "scalar"))
_solve_poly_case("out_given", out="given", max_iter=4, tol=1e-5)
_solve_poly_case("out_list", out="list")
_solve_poly_case("err_out_pair", out="pair")
_solve_poly_case("err_out_shape", out="shape")
_solve_poly_case("err_out_dtype", out="dtype")
_solve_poly_case("err_out_strided", out="strided")
_solve_poly_case("err_rows_width", rows="wide")
_solve_poly_case("err_rows_dims", rows="3d")
_solve_poly_case("err_rows_mixed", rows=("shared", "per"))
_solve_poly_case("err_rows_batches", rows=("per", "per2"))
_solve_poly_case("err_rows_vs_f_batch", rows=("per2", "none"))
_solve_poly_case("err_box_per", box="per")


@case
def solve_poly_err_f_dims(c):
    return bt.solve_poly(T(6), T(1, 2, 3))


@case
def solve_poly_err_H_dims(c):
    return bt.solve_poly(T(2, 6), T(2, 3))


@case
def solve_poly_err_H_size(c):
    return bt.solve_poly(T(5), T(2, 3))


@case
def solve_poly_err_G(c):
    return bt.solve_poly(T(6), T(2, 3), T(2, 4))


def _qp(c, G=True, F=True, box="scalar", n=3, m=2, nx=2):
    lbz, ubz = bounds(c, box, n, 1, names=("lbz", "ubz"))
    return bt.PolyQP(c.inp("H", T(n * (n + 1) // 2)), c.inp("G", T(m, n, k=3)) if G else None,
                     c.inp("Fm", T(n, nx, k=4)) if F else None, lbz, ubz)


@case
def polyqp_init(c):
    return _qp(c)


@case
def polyqp_init_bare(c):
    return _qp(c, G=False, F=False, box="none")


@case
def polyqp_init_box_shared(c):
    return _qp(c, box=("shared", "none"))


@case
def polyqp_init_dtype_device(c):
    return bt.PolyQP(c.inp("H", T(6)), dtype=F32, device=torch.device("cpu"))


@case
def polyqp_init_err_H(c):
    return bt.PolyQP(T(2, 6))


@case
def polyqp_init_err_G(c):
    return bt.PolyQP(T(6), T(2, 4))


@case
def polyqp_init_err_F(c):
    return bt.PolyQP(T(6), None, T(4, 2))


@case
def polyqp_init_err_box(c):
    return bt.PolyQP(T(6), None, None, T(2, 3))


def _poly_solve_case(name, x0="per", fv=None, rows="shared", out=None, F=True, G=True,
                     box="scalar", **kw):
    def f(c):
        n, m, nx, b = 3, 2, 2, 2
        qp = _qp(c, G=G, F=F, box=box)
        x = None if x0 is None else c.inp("x0", T(*((b, nx) if x0 == "per" else (nx,))))
        fz = None if fv is None else c.inp("f", T(*((b, n) if fv == "per" else (n,)), k=2))
        hl, hu = _rows(c, rows, m if G else 0, b)
        return qp.solve(x, fz, hl, hu, out=_poly_out_arg(c, out, b, n, qp.mt), **kw)
    f.__name__ = "polyqp_solve_" + name
    case(f)


_poly_solve_case("plain")
_poly_solve_case("shared_x0_per_f", x0="shared", fv="per", rows="none")
_poly_solve_case("f_only_rows_per", x0=None, fv="shared", rows="per", F=False)
_poly_solve_case("all_shared", x0="shared", fv="shared")
_poly_solve_case("rows_hu_only", rows=("none", "per"))
_poly_solve_case("out_given", out="given", max_iter=6, tol=1e-4)
_poly_solve_case("err_x0_without_F", F=False)
_poly_solve_case("err_rows_mixed", rows=("per", "shared"))
_poly_solve_case("err_out_shape", out="shape")
_poly_solve_case("err_out_pair", out="pair")
_poly_solve_case("err_batch", rows="per2")


@case
def polyqp_solve_err_f_width(c):
    return _qp(c).solve(T(2, 2), T(2, 4))


@case
def polyqp_affine_scratch_bytes(c):
    return _qp(c).affine_scratch_bytes(5, 7, True)


def _poly_loop_case(name, rows="shared", E=True, w=False, soft=None, g=None, e=None, out=None,
                    G=True, steps=4, bad=None, **kw):
    def f(c):
        n, nx, nu, b = 3, 2, 1, 2
        m = 2 if G else 0
        qp = _qp(c, G=G, box="scalar")
        A, B = c.inp("A", T(nx, nx)), c.inp("B", T(nx, nu, k=2))
        x = c.inp("x0", T(b, nx))
        hl, hu = _rows(c, rows, m, b)
        Em = c.inp("E", T(m, nx, k=5)) if E and G else None
        k = dict(kw)
        if w:
            k["w"] = c.inp("w", T(steps, b, nx))
        if soft == "scalar":
            k["soft"] = (10.0, 0.5)
        elif soft == "vector":
            k["soft"] = (c.inp("rho", T(m, k=10)), c.inp("sigma", torch.tensor(0.5, dtype=F64)))
        elif soft is not None:
            k["soft"] = soft
        if g is not None:
            k["g"] = c.inp("g", T(*((steps, b, n) if g == "per" else (steps, n)), k=6))
        if e is not None:
            k["e"] = c.inp("e", T(*((steps, b, m) if e == "per" else (steps, m)), k=7))
        if out == "scratch":
            k["out"] = {"scratch": c.inp("out.scratch", torch.empty((2 * WS_BYTES,), dtype=torch.uint8)),
                        "xs": c.inp("out.xs", torch.empty((steps + 1, b, nx), dtype=F64))}
        elif out == "small_scratch":
            k["out"] = {"scratch": torch.empty((8,), dtype=torch.uint8)}
        elif out == "bad_xs":
            k["out"] = {"xs": torch.empty((steps, b, nx), dtype=F64)}
        elif out == "bad_status":
            k["out"] = {"status": torch.empty((steps, b), dtype=torch.int64)}
        elif out == "some":
            k["out"] = {"us": c.inp("out.us", torch.empty((steps, b, nu), dtype=F64)),
                        "zs": c.inp("out.zs", torch.empty((steps, b, n), dtype=F64))}
        if bad == "A":
            A = T(nx, nx + 1)
        if bad == "B":
            B = T(nx + 1, nu)
        if bad == "nu":
            B = T(nx, n + 1)
        if bad == "x0":
            x = T(nx)
        if bad == "E":
            Em = T(m, nx + 1)
        if bad == "w":
            k["w"] = T(steps, b + 1, nx)
        if bad == "g":
            k["g"] = T(steps + 1, n)
        if bad == "e":
            k["e"] = T(steps, b, m + 1)
        return qp.loop(A, B, x, steps, hl, hu, Em, **k)
    f.__name__ = "polyqp_loop_" + name
    case(f)


_poly_loop_case("hard")
_poly_loop_case("hard_rows_per_w_cold", rows="per", w=True, cold=True, plans=True,
                multipliers=True, max_iter=8, tol=1e-3)
_poly_loop_case("hard_rows_hl_only", rows=("shared", "none"), E=False)
_poly_loop_case("hard_out_some", out="some", plans=True)
_poly_loop_case("soft_scalar", soft="scalar", slacks=True)
_poly_loop_case("soft_vector", soft="vector", rows="per")
_poly_loop_case("soft_m0", soft="scalar", G=False, rows="none")
_poly_loop_case("affine_g_shared", g="shared")
_poly_loop_case("affine_g_per", g="per", w=True, cold=True)
_poly_loop_case("affine_e_only", e="shared")
_poly_loop_case("affine_e_per_g_shared", g="shared", e="per", multipliers=True)
_poly_loop_case("affine_soft", g="per", soft="scalar", slacks=True, plans=True)
_poly_loop_case("affine_soft_m0", g="shared", soft="scalar", G=False, rows="none")
_poly_loop_case("affine_scratch_given", g="shared", out="scratch")
_poly_loop_case("zero_steps", steps=0)
_poly_loop_case("err_A", bad="A")
_poly_loop_case("err_B", bad="B")
_poly_loop_case("err_nu", bad="nu")
_poly_loop_case("err_x0", bad="x0")
_poly_loop_case("err_steps", steps=-1)
_poly_loop_case("err_hl_width", rows=("wide", "none"))
_poly_loop_case("err_hu_batch", rows=("none", "per2"))
_poly_loop_case("err_rows_mixed", rows=("shared", "per"))
_poly_loop_case("err_E", bad="E")
_poly_loop_case("err_w", bad="w")
_poly_loop_case("err_g", bad="g")
_poly_loop_case("err_e", bad="e")
_poly_loop_case("err_soft_pair", soft=(1.0,))
_poly_loop_case("err_soft_shape", soft=(T(3), 1.0))
_poly_loop_case("err_slacks", slacks=True)
_poly_loop_case("err_scratch", g="shared", out="small_scratch")
_poly_loop_case("err_out_shape", out="bad_xs")
_poly_loop_case("err_out_dtype", out="bad_status")
_poly_loop_case("err_A_then_steps", bad="A", steps=-1)


@case
def polyqp_loop_err_no_F(c):
    return _qp(c, F=False).loop(T(2, 2), T(2, 1), T(2, 2), 3)


# ---- tracking_terms / mpc_poly_loop
def _tracking_case(name, gam=(6, 3), x_ref=None, u_ref=None, N=3, steps=2):
    def f(c):
        nx, nu = 2, 1
        xr = None if x_ref is None else T(*x_ref, k=2)
        ur = None if u_ref is None else T(*u_ref, k=3)
        return bt.tracking_terms({"Gam": T(*gam)}, T(nx, nx), T(nu, nu), T(nx, nx, k=2), N, steps,
                                 xr, ur)
    f.__name__ = "tracking_terms_" + name
    case(f, values=True)


_tracking_case("setpoint", x_ref=(2,))
_tracking_case("trajectory_both", x_ref=(6, 2), u_ref=(5, 1))
_tracking_case("per_reference", x_ref=(4, 6, 2), u_ref=(1,))
_tracking_case("per_gam", gam=(4, 6, 3), x_ref=(4, 6, 2), u_ref=(5, 1))
_tracking_case("u_only", u_ref=(5, 1))
_tracking_case("err_gam", gam=(3,), x_ref=(2,))
_tracking_case("err_none")
_tracking_case("err_window", x_ref=(5, 2))
_tracking_case("err_batches", x_ref=(4, 6, 2), u_ref=(3, 5, 1))
_tracking_case("err_gam_batch", gam=(3, 6, 3), x_ref=(4, 6, 2))


def _poly_loop_fn_case(name, per="", xlo="stage", lb="scalar", soft=None, ref=False, plant_=False,
                       **kw):
    def f(c):
        nx, nu, N, b, steps = 2, 1, 3, 2, 3
        ops = plant(c, nx, nu, N, b, per)
        x = c.inp("x0", T(b, nx))
        lo = {"none": None, "stage": c.inp("xlo", T(nx, k=-1)), "rows": c.inp("xlo", T(N * nx, k=-1)),
              "bad": T(nx + 1)}[xlo]
        hi = None if xlo == "none" else 5.0
        k = dict(kw)
        if soft is not None:
            k["soft"] = soft
        if ref:
            k["x_ref"] = c.inp("x_ref", T(nx))
        if plant_:
            k["plant"] = (c.inp("Ap", T(nx, nx, k=7)), c.inp("Bp", T(nx, nu, k=8)))
        return bt.mpc_poly_loop(*ops, N, x, lo, hi, -1.0 if lb == "scalar" else None, 1.0, steps,
                                **k)
    f.__name__ = "mpc_poly_loop_" + name
    case(f)


_poly_loop_fn_case("plain")
_poly_loop_fn_case("rows_soft", xlo="rows", soft=(10.0, T(2, k=0.5)), slacks=True)
_poly_loop_fn_case("no_state_box_ref_plant", xlo="none", ref=True, plant_=True, plans=True)
_poly_loop_fn_case("err_per_model", per="A")
_poly_loop_fn_case("err_stage_bound", xlo="bad")
_poly_loop_fn_case("err_soft_pair", soft=(1.0, 2.0, 3.0))
_poly_loop_fn_case("err_soft_without_box", xlo="none", soft=(1.0, 2.0))


# ---- general QP, sweep, Riccati, gemv, rollout
def _solve_qp_case(name, hper=True, fper=True, G="shared", rows="shared", form="scalar", out=False,
                   ws=False, **kw):
    def f(c):
        n, m, b = 3, 2, 2
        H = c.inp("H", T(*((b,) if hper else ()) + (6,)))
        fv = c.inp("f", T(*((b,) if fper else ()) + (n,), k=2))
        Gm = {"none": None, "shared": (m, n), "per": (b, m, n), "4d": (1, b, m, n)}[G]
        Gm = None if Gm is None else c.inp("G", T(*Gm, k=3))
        hl, hu = _rows(c, rows, m, b)
        lb, ub = bounds(c, form, n, b)
        k = dict(kw)
        if out:
            k["out"] = (c.inp("out.z", torch.empty((b, n), dtype=F64)),
                        c.inp("out.y", torch.empty((b, m), dtype=F64)),
                        c.inp("out.status", torch.empty((b,), dtype=I32)))
        if ws:
            k["ws"] = c.inp("ws", torch.empty((WS_BYTES,), dtype=torch.uint8))
        return bt.solve_qp(H, fv, Gm, hl, hu, lb, ub, **k)
    f.__name__ = "solve_qp_" + name
    case(f)


for _f in BOUND_FORMS:
    _solve_qp_case("bounds_" + _form_name(_f), form=_f)
_solve_qp_case("all_shared", hper=False, fper=False, form="shared")
_solve_qp_case("per_G_rows", G="per", rows="per")
_solve_qp_case("no_G", G="none", rows="none")
_solve_qp_case("hl_only_per", rows=("per", "none"))
_solve_qp_case("hu_only", rows=("none", "shared"))
_solve_qp_case("out_ws", out=True, ws=True, max_iter=12, tol=1e-11)
_solve_qp_case("no_presweep", presweep=False)
_solve_qp_case("err_rows_shapes", rows=("shared", "per"))
_solve_qp_case("err_rows_dims", rows="3d")
_solve_qp_case("err_G_dims", G="4d")
_solve_qp_case("err_rows_batch", rows="per2")


@case
def solve_qp_err_packed(c):
    return bt.solve_qp(T(2, 7), T(2, 3))


@case
def solve_qp_err_packed_then_rows(c):
    return bt.solve_qp(T(2, 7), T(2, 3), T(2, 3), T(2), T(2, 2))


@case
def sweep_per(c):
    return bt.sweep(c.inp("H", T(2, 6, dt=F32)), c.inp("G", T(2, 2, 3, dt=F32)))


@case
def sweep_shared_full(c):
    return bt.sweep(c.inp("H", T(6, dt=F32)), full=True)


@case
def sweep_err_batch(c):
    return bt.sweep(T(2, 6, dt=F32), T(3, 2, 3, dt=F32))


@case
def riccati_shared(c):
    A, B, Q, R, Qf = plant(c)
    return bt.riccati(A, B, Q, R, Qf, 3)


@case
def riccati_per(c):
    A, B, Q, R, Qf = plant(c, per="A Qf")
    return bt.riccati(A, B, Q, c.inp("R1", T(1)), Qf, 3)


@case
def riccati_err_dims(c):
    A, B, Q, R, Qf = plant(c)
    return bt.riccati(A, B, T(1, 2, 2, 2), R, Qf, 3)


@case
def gemv_shared(c):
    return bt.gemv(c.inp("M", T(3, 2)), c.inp("x", T(4, 2)), 2.0, 0.5)


@case
def gemv_per_y(c):
    return bt.gemv(c.inp("M", T(4, 3, 2)), c.inp("x", T(2)), y=c.inp("y", T(4, 3)))


@case
def gemv_err_batch(c):
    return bt.gemv(T(4, 3, 2), T(3, 2))


@case
def rollout_plain(c):
    return bt.rollout(c.inp("A", T(2, 2)), c.inp("B", T(2, 1)), c.inp("K", T(1, 2)),
                      c.inp("x0", T(5, 2)), 7)


# ---- bicycle
PRM = types.SimpleNamespace(axis_front=1.5, axis_rear=1.25, acceleration=3.0, friction=0.1)
PRM2 = types.SimpleNamespace(axis_front=1.0, axis_rear=2.0, acceleration=4.0, friction=0.2)


@case
def bicycle_rti_plain(c):
    return bt.bicycle_rti(c.inp("x0", T(2, 4)), c.inp("U", T(2, 3, 2)), PRM, 0.05)


@case
def bicycle_rti_states_strided(c):
    return bt.bicycle_rti(c.inp("x0", T(2, 4, dt=F32)), T(3, 2, 2, dt=F32).transpose(0, 1), PRM,
                          0.05, states=True)


@case
def bicycle_linearise_plain(c):
    return bt.bicycle_linearise(c.inp("x0", T(2, 4)), c.inp("U", T(2, 3, 2)), PRM, 0.05)


@case
def bicycle_linearise_out(c):
    out = (c.inp("out.A", torch.empty((2, 3, 4, 4), dtype=F64)),
           c.inp("out.B", torch.empty((2, 3, 4, 2), dtype=F64)),
           c.inp("out.c", torch.empty((2, 3, 4), dtype=F64)),
           c.inp("out.X", torch.empty((2, 4, 4), dtype=F64)))
    return bt.bicycle_linearise(c.inp("x0", T(2, 4)), c.inp("U", T(2, 3, 2)), PRM, 0.05, 1, out)


def _hessian_case(name, Q=False, out=False, extras=False, **kw):
    def f(c):
        b, N = 2, 3
        X, U, pi = c.inp("X", T(b, N + 1, 4)), c.inp("U", T(b, N, 2)), c.inp("pi", T(b, N, 4))
        k = dict(kw)
        if extras:
            k.update(flags=c.inp("flags", torch.zeros(b, dtype=I32)), mu=c.inp("mu", T(b)),
                     fix=c.inp("fix", torch.zeros((b, N), dtype=I32)))
        if Q:
            k.update(Q=c.inp("Q", T(4, 4)), R=c.inp("R", T(2, 2, dt=F32)))
        if out:
            k["out"] = (c.inp("out.H2", torch.empty((b, N, 6, 6), dtype=F64)),
                        c.inp("out.q2", torch.empty((b, N, 6), dtype=F64)))
        return bt.bicycle_hessian(X, U, pi, PRM, 0.05, **k)
    f.__name__ = "bicycle_hessian_" + name
    case(f)


_hessian_case("plain")
_hessian_case("extras_out", extras=True, out=True, integrator=1)
_hessian_case("convex", Q=True, eps=1e-4)
_hessian_case("convex_extras_out", Q=True, extras=True, out=True, integrator=1)


def _sqp_state(c, b, N, fix=True):
    st = {"rho": c.inp("st.rho", T(b)), "kkt": c.inp("st.kkt", T(b, k=2)),
          "mu": c.inp("st.mu", T(b, k=3)), "flags": c.inp("st.flags", torch.zeros(b, dtype=I32))}
    if fix:
        st["fix"] = c.inp("st.fix", torch.zeros((b, N), dtype=I32))
    return st


def _pair(c, form, b, width, names):
    def one(name, f, k):
        shp = {"none": None, "shared": (width,), "per": (b, width), "bad": (width + 1,)}[f]
        return None if shp is None else c.inp(name, T(*shp, k=k))
    lo, hi = form if isinstance(form, tuple) else (form, form)
    return one(names[0], lo, -1), one(names[1], hi, 1)


def _sqp_step_case(name, xform="shared", uform="shared", fix=True, **kw):
    def f(c):
        b, N = 2, 3
        xlo, xhi = _pair(c, xform, b, 4 * N, ("xlo", "xhi"))
        lb, ub = _pair(c, uform, b, 2 * N, ("lb", "ub"))
        return bt.bicycle_sqp_step(
            c.inp("x0", T(b, 4)), c.inp("U", T(b, N, 2)), c.inp("Z", T(b, N * 2)),
            c.inp("yq", T(b, N * 4)), c.inp("piq", T(b, N, 4)), c.inp("y", T(b, N * 4, k=2)),
            c.inp("pi", T(b, N, 4, k=2)), c.inp("X", T(b, N + 1, 4)), _sqp_state(c, b, N, fix),
            PRM, 0.05, c.inp("Q", T(4, 4)), c.inp("R", T(2, 2)), c.inp("Qf", T(4, 4, k=2)),
            xlo, xhi, lb, ub, **kw)
    f.__name__ = "bicycle_sqp_step_" + name
    case(f)


_sqp_step_case("shared")
_sqp_step_case("per_no_fix", xform="per", uform="per", fix=False, tol=1e-6, integrator=1)
_sqp_step_case("mixed_broadcast", xform=("shared", "per"), uform=("per", "shared"))
_sqp_step_case("none_and_one_side", xform="none", uform=("none", "shared"))
_sqp_step_case("err_pair", xform="bad")
_sqp_step_case("err_pair_u", uform=("shared", "bad"))


@case
def bicycle_sqp_step_qp_status(c):
    b, N = 2, 3
    return bt.bicycle_sqp_step(
        c.inp("x0", T(b, 4)), c.inp("U", T(b, N, 2)), c.inp("Z", T(b, N * 2)),
        c.inp("yq", T(b, N * 4)), c.inp("piq", T(b, N, 4)), c.inp("y", T(b, N * 4, k=2)),
        c.inp("pi", T(b, N, 4, k=2)), c.inp("X", T(b, N + 1, 4)), _sqp_state(c, b, N), PRM, 0.05,
        c.inp("Q", T(4, 4)), c.inp("R", T(2, 2)), c.inp("Qf", T(4, 4, k=2)),
        qp_status=c.inp("qp_status", torch.zeros(b, dtype=I32)))


def _sqp_solve_case(name, xform="shared", uform="per", ws=False, extras=False, bad=None, **kw):
    def f(c):
        b, N = 2, 3
        xlo, xhi = _pair(c, xform, b, 4 * N, ("xlo", "xhi"))
        lb, ub = _pair(c, uform, b, 2 * N, ("lb", "ub"))
        t = {"x0": T(b, 4), "U": T(b, N, 2), "y": T(b, N * 4), "pi": T(b, N, 4),
             "X": T(b, N + 1, 4)}
        if bad == "y":
            t["y"] = T(b, N, 4)
        if bad == "X":
            t["X"] = T(b, N + 1, 4, dt=F32)
        if bad == "pi":
            t["pi"] = T(b, 4, N).transpose(1, 2)
        t = {k: c.inp(k, v) for k, v in t.items()}
        k = dict(kw)
        if ws:
            k["ws"] = c.inp("ws", torch.empty((WS_BYTES,), dtype=torch.uint8))
        if extras:
            k.update(lam_u=c.inp("lam_u", T(b, N * 2)),
                     qp_status=c.inp("qp_status", torch.zeros(b, dtype=I32)))
        return bt.bicycle_sqp_solve(t["x0"], t["U"], t["y"], t["pi"], t["X"], _sqp_state(c, b, N),
                                    PRM, 0.05, c.inp("Q", T(4, 4)), c.inp("R", T(2, 2)),
                                    c.inp("Qf", T(4, 4, k=2)), xlo=xlo, xhi=xhi, lb=lb, ub=ub, **k)
    f.__name__ = "bicycle_sqp_solve_" + name
    case(f)


_sqp_solve_case("plain")
_sqp_solve_case("ws_extras", ws=True, extras=True, hessian="gauss-newton", tol=1e-7, max_iter=9,
                qp_max_iter=4, integrator=1)
_sqp_solve_case("mixed", xform=("per", "shared"), uform="none", hessian="exact-raw")
_sqp_solve_case("err_y", bad="y")
_sqp_solve_case("err_X_dtype", bad="X")
_sqp_solve_case("err_pi_strided", bad="pi")
_sqp_solve_case("err_pair_then_y", xform="bad", bad="y")


def _bike_loop_case(name, xform="shared", uform="per", ws=False, bad=None, **kw):
    def f(c):
        b, N, T_ = 2, 3, 4
        xlo, xhi = _pair(c, xform, b, 4 * N, ("xlo", "xhi"))
        lb, ub = _pair(c, uform, b, 2 * N, ("lb", "ub"))
        t = {"xs": T(T_ + 1, b, 4), "us": T(T_, b, 2),
             "success": torch.zeros((T_, b), dtype=torch.bool),
             "iters": torch.zeros((T_, b), dtype=I32), "state_prediction": T(T_, b, N + 1, 4),
             "input_prediction": T(T_, b, N, 2)}
        if bad == "xs":
            t["xs"] = T(T_, b, 4)
        if bad == "success":
            t["success"] = torch.zeros((T_, b), dtype=I32)
        if bad == "input_prediction":
            t["input_prediction"] = T(T_, b, 2, N).transpose(2, 3)
        t = {k: c.inp(k, v) for k, v in t.items()}
        k = dict(kw)
        if ws:
            k["ws"] = c.inp("ws", torch.empty((WS_BYTES,), dtype=torch.uint8))
        return bt.bicycle_mpc_loop(
            t["xs"], t["us"], t["success"], t["iters"], t["state_prediction"],
            t["input_prediction"], c.inp("U", T(b, N, 2)), c.inp("y", T(b, N * 4)),
            c.inp("pi", T(b, N, 4)), c.inp("X", T(b, N + 1, 4)), _sqp_state(c, b, N), PRM, 0.05,
            c.inp("Q", T(4, 4)), c.inp("R", T(2, 2)), c.inp("Qf", T(4, 4, k=2)),
            plant_params=PRM2, xlo=xlo, xhi=xhi, lb=lb, ub=ub, **k)
    f.__name__ = "bicycle_mpc_loop_" + name
    case(f)


_bike_loop_case("plain")
_bike_loop_case("ws_knobs", ws=True, plant=2, substeps=5, hessian="gauss-newton", tol=1e-6,
                iters_first=30, iters_per_step=3, qp_max_iter=7, integrator=1, mu0=1e-2)
_bike_loop_case("mixed", xform=("shared", "per"), uform=("none", "per"))
_bike_loop_case("err_xs", bad="xs")
_bike_loop_case("err_success_dtype", bad="success")
_bike_loop_case("err_prediction_strided", bad="input_prediction")
_bike_loop_case("err_pair_then_xs", uform="bad", bad="xs")


# ---- functions without a library call, and the seams' own checks
@case(values=True)
def pack_lower_values(c):
    return bt.pack_lower(T(2, 3, 3))


@case(values=True)
def unpack_lower_values(c):
    return bt.unpack_lower(T(2, 6), 3)


@case(values=True)
def unpack_gam_values(c):
    return bt.unpack_gam(T(1, 12), 3, 2, 1)


@case(values=True)
def status_code_and_iters(c):
    s = torch.tensor([0, 257, (7 << 8) | 3 | (1 << 24)], dtype=I32)
    return bt.status_code(s), bt.status_iters(s)


@case
def workspace_queries(c):
    return (bt.workspace_bytes(F32, 8, 70), bt.workspace_bytes(F64, 8, 20, 5),
            bt.mpc_qp_workspace_bytes(F32, 4, 2, 1, 10), bt.max_qp_size(F32), bt.n_packed(5),
            bt.isqrt_packed(15))


@case
def seam_workspace_err(c):
    return _ORIG["_workspace"](64, torch.device("cpu"), torch.empty((128,), dtype=torch.uint8))


@case
def seam_workspace_none(c):
    return _ORIG["_workspace"](0, torch.device("cpu"))


@case
def seam_dev_err(c):
    return _ORIG["_dev"](T(2), F64, torch.device("cpu"))


@case
def seam_dev_none(c):
    return _ORIG["_dev"](None, F64, torch.device("cpu"))


@case
def helper_weight_r(c):
    return bt._weight_r(c.inp("R", T(1)), 1), bt._weight_r(c.inp("R2", T(2, 2)), 2)


@case
def helper_bound_pair(c):
    lo, hi = c.inp("lo", T(4)), c.inp("hi", T(3, 4))
    return (bt._bound_pair(lo, None, 3, 4, "x"), bt._bound_pair(lo, hi, 3, 4, "x"),
            bt._bound_pair(None, None, 3, 4, "x"))


if __name__ == "__main__":
    with open(sys.argv[1], "w") as fh:
        json.dump({"parent": sys.argv[2], "cases": record_all()}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{len(CASES)} cases written to {sys.argv[1]}")
