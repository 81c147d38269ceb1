"""Shared cases of the stage-wise interior point (test_ipm_host.py on the host
build of solve_lane, test_gpu_ipm.py on every kernel): a time-varying (4, 2)
batch with its oracle solution, and the three inputs that drive the iteration
control into MAXITER, strict NOT_CONVEX and NONFINITE."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

from oracle import condense as oc
from oracle import qp as oq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NU, N, BATCH = 4, 2, 12, 16
DT = 0.2
Q = np.diag([1.0, 2.0, 0.1, 0.1])
R = np.diag([0.1, 0.05])
QF = 5.0 * Q
XHI = np.array([2.5, 2.5, 1.0, 1.0])
UHI = np.ones(NU)
STRICT = 6  # inertia corrections of a strict QP (mpcqp_mpc_ipm's default)


@functools.lru_cache(maxsize=None)
def tv_batch():
    """Double integrator in two axes (dt = 0.2), every stage matrix perturbed:
    A_k, B_k, c_k, x0 per instance, state box +-(2.5, 2.5, 1, 1), inputs +-1."""
    rng = np.random.default_rng(7)
    A0 = np.eye(NX)
    A0[0, 2] = A0[1, 3] = DT
    B0 = np.zeros((NX, NU))
    B0[0, 0] = B0[1, 1] = 0.5 * DT * DT
    B0[2, 0] = B0[3, 1] = DT
    A = np.empty((BATCH, N, NX, NX))
    B = np.empty((BATCH, N, NX, NU))
    c = np.empty((BATCH, N, NX))
    x0 = np.empty((BATCH, NX))
    for i in range(BATCH):
        A[i] = A0 + 0.03 * rng.standard_normal((N, NX, NX))
        B[i] = B0 + 0.02 * rng.standard_normal((N, NX, NU))
        c[i] = 0.05 * rng.standard_normal((N, NX))
        x0[i] = rng.uniform(-1, 1, NX) * np.array([2.2, 2.2, 0.8, 0.8])
    out = dict(A=A, B=B, c=c, x0=x0)
    for v in out.values():
        v.setflags(write=False)
    return out


def solve_oracle(A, B, c, x0, Q=Q, R=R, QF=QF, xhi=XHI, uhi=UHI):
    """Condensed QP of every instance by the oracle's active set: z, X, the
    state-row multipliers y (> 0 at xhi), the input-bound multipliers, the
    condensed data, and the number of active state and input rows."""
    res = dict(z=[], X=[], y=[], lam_u=[], d=[], act_x=[], act_u=[])
    n = A.shape[1]
    for i in range(A.shape[0]):
        d = oc.condense(A[i], B[i], Q, R, QF, n, x0=x0[i], c=c[i])
        G = np.vstack([d["Gam"], -d["Gam"]])
        h = np.concatenate([np.tile(xhi, n) - d["xbar"], np.tile(xhi, n) + d["xbar"]])
        ub = np.tile(uhi, n)
        z, lam, _ = oq.poly_qp(d["H"], d["f"], G, h, -ub, ub)  # raises if not solved
        m = n * A.shape[-1]
        y = lam[:m] - lam[m:2 * m]
        X = d["xbar"] + d["Gam"] @ z
        res["z"].append(z)
        res["X"].append(X)
        res["y"].append(y)
        res["lam_u"].append(-(d["H"] @ z + d["f"] + d["Gam"].T @ y))
        res["d"].append(d)
        res["act_x"].append(int((np.abs(np.abs(X) - np.tile(xhi, n)) < 1e-9).sum()))
        res["act_u"].append(int((np.abs(np.abs(z) - ub) < 1e-9).sum()))
    for k in ("z", "X", "y", "lam_u"):
        res[k] = np.stack(res[k])
        res[k].setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def tv_oracle():
    return solve_oracle(**tv_batch())


def h2_nonconvex(batch=BATCH, n=N):
    """Extra stage cost with -1e3 on both input diagonals of every stage: no
    inertia correction a strict QP may take makes the reduced Hessian positive."""
    H2 = np.zeros((batch, n, NX + NU, NX + NU))
    H2[:, :, NX, NX] = H2[:, :, NX + 1, NX + 1] = -1e3
    return H2


def x0_nan(x0, inst=1):
    x = np.array(x0)
    x[inst, 1] = np.nan
    return x


# ------------------------------------------------------------- the host build
def build_host(tmp_path):
    """tools/ipm_host.cpp (solve_lane for the CPU) compiled without contraction;
    None without a compiler."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    so = os.path.join(str(tmp_path), "libipm_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "ipm_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def host_solve(lib, A, B, Q, R, QF, x0, n, c=None, xlo=None, xhi=None, lb=None, ub=None,
               H2=None, max_iter=100, tol=1e-10, strict=None):
    """ipm_host_solve on a batch; A, B shared (2-D) or per instance and stage
    (4-D); bounds one stage's, shared by all stages and instances; H2 one
    instance's, shared.  strict: the tool's STRICT knob, read at every call."""
    dp = ctypes.POINTER(ctypes.c_double)
    keep = []

    def p(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(dp)

    batch, nx = x0.shape
    nu = np.shape(B)[-1]
    tv = int(np.ndim(A) == 4)
    sA, sB = (n * nx * nx, n * nx * nu) if tv else (0, 0)
    til = lambda v, r: None if v is None else np.tile(np.asarray(v, float), r)  # noqa: E731
    z = np.zeros((batch, n * nu))
    y, X, pi = (np.zeros((batch, n * nx)) for _ in range(3))
    st = np.zeros(batch, np.int32)
    old = os.environ.pop("STRICT", None)
    if strict is not None:
        os.environ["STRICT"] = str(strict)
    try:
        lib.ipm_host_solve(
            ctypes.c_int(batch), ctypes.c_int(nx), ctypes.c_int(nu), ctypes.c_int(n),
            ctypes.c_int(tv), p(A), ctypes.c_long(sA), p(B), ctypes.c_long(sB), p(c),
            ctypes.c_long(n * nx if c is not None else 0), p(Q), p(R), p(QF), p(x0),
            p(til(xlo, n)), p(til(xhi, n)), p(til(lb, n)), p(til(ub, n)), p(z), p(y), p(X),
            st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.c_int(max_iter),
            ctypes.c_double(tol), p(H2), None, p(pi))
    finally:
        os.environ.pop("STRICT", None)
        if old is not None:
            os.environ["STRICT"] = old
    return dict(z=z, y=y, X=X, pi=pi, status=st)


def host_runs(lib, golden):
    """Every run the host tests make, by name: (2,1) golden, (4,2) batch, and
    the three ladder cases on that batch."""
    g = golden("boxqp_cfg2.npz")
    t = tv_batch()
    kw = dict(c=t["c"], xlo=-XHI, xhi=XHI, lb=-UHI, ub=UHI)
    return dict(
        cfg2=host_solve(lib, g["A"], g["B"], g["Q"], g["R"], g["Pf"], g["x0"], int(g["N"]),
                        lb=[-1.0], ub=[1.0]),
        tv=host_solve(lib, t["A"], t["B"], Q, R, QF, t["x0"], N, **kw),
        maxiter=host_solve(lib, t["A"], t["B"], Q, R, QF, t["x0"], N, max_iter=2, **kw),
        notconvex=host_solve(lib, t["A"], t["B"], Q, R, QF, t["x0"], N, H2=h2_nonconvex(1),
                             strict=STRICT, **kw),
        nan=host_solve(lib, t["A"], t["B"], Q, R, QF, x0_nan(t["x0"]), N, **kw),
    )
