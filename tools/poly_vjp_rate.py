"""Time of the polytope-QP adjoint (mpcqp_poly_solve_vjp) next to the forward
solve and next to what exists without it.

  python tools/poly_vjp_rate.py [--repeats 20] [--json profiles/poly_vjp/rate.json]

Two shapes, fp64:

  config4   BASELINE config 4, the data recipe of tests/_poly_loop_cases.py
            config4_problem: nx = 12, nu = 4, N = 50 (n = 200), 40 random rows
            G z <= hu, no box, x0 ~ 3 N(0, 1); B = 131,072;
  session2  the session-2 MPC (problems.Problem) at N = 20: state box on
            x_1..x_N (40 rows) and input box (m_total = 60), x0 spread over the
            feasible part of the state box; B = 4096.

gz and gy are standard normal.  Each (shape, step) is a child process of its own
under its own time limit (a step that fails or runs out of time ends the run),
timed with HIP events around one call, warm-up first, the median of --repeats:

  vjp      "together": mpcqp_poly_solve_vjp with gz, gy and all four outputs
           into buffers allocated beforehand, both launches; "product" and
           "adjoint": the device time of each of the two kernels
           (poly_affine_prep_kernel, poly_vjp_kernel) in --repeats further
           calls, as torch.profiler records it; "wrapper":
           poly_diff.poly_solve_vjp, which also allocates;
  forward  mpcqp_poly_solve (PolyQP.solve) on the same batch;
  torch    the same gradients from batched torch ops: per instance the dense
           KKT system [[H, (D C)'], [D C, I - D]] [dz; e] = [gz; D gy], D the
           active rows, by torch.linalg.solve.  The systems take (n + m_total)^2
           doubles each, so this step runs on --torch-batch instances (1024)
           in chunks of --torch-chunk systems per call, and reports the time per
           instance as well; where the library's batched LU refuses a chunk (its
           workspace is of fixed size) the systems are solved one by one, and
           "solve_mode" says so.

No threshold is asserted.  Prints one JSON line and writes it to --json.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from model_predictive_control_amd import _native as nat  # noqa: E402
from model_predictive_control_amd import batched, poly_diff  # noqa: E402
from model_predictive_control_amd.problems import Problem  # noqa: E402

STEPS = ("vjp", "forward", "torch")
SHAPES = {"config4": 131072, "session2": 4096}
OUTS = ("gf", "gx0", "ghl", "ghu")


def _median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def _kernel_ms(fn, repeats):
    """Device time of the two kernels of one call, each the median over
    ``repeats`` calls, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
    out = {}
    for key, name in (("product", "poly_affine_prep_kernel"), ("adjoint", "poly_vjp_kernel")):
        ts = [e.device_time * 1e-3 for e in prof.events() if name in e.name]
        assert len(ts) == repeats, (name, len(ts))
        out[key] = dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)),
                        max_ms=float(np.max(ts)))
    return out


def _problem(shape, batch, dev):
    """(qp, solve arguments (x0, f, hl, hu), dense H, C = [G; I], F)."""
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)  # noqa: E731
    if shape == "config4":
        nx, nu, N, m = 12, 4, 50, 40
        rng = np.random.default_rng(nx * 100 + N)
        U, _ = np.linalg.qr(rng.normal(size=(nx, nx)))
        A = (U * rng.uniform(0.5, 0.98, nx)) @ U.T
        B = rng.normal(size=(nx, nu)) / np.sqrt(nx)
        cd = batched.condense(t(A), t(B), t(np.eye(nx)), t(0.1 * np.eye(nu)), t(np.eye(nx)), N,
                              outputs=("H", "F"))
        G = t(rng.normal(size=(m, N * nu)))
        hu = t(rng.uniform(0.5, 1.5, size=m))
        x0 = t(rng.normal(size=(batch, nx)) * 3)
        qp = batched.PolyQP(cd["H"][0], G, cd["F"][0])
        args = (x0, None, None, hu)
    else:
        p, N = Problem(), 20
        cd = batched.condense(t(p.A), t(p.B), t(p.Q), t(p.R), t(p.Q), N,
                              outputs=("H", "F", "Gam", "Phi"))
        rng = np.random.default_rng(20)
        x0 = t(np.column_stack([rng.uniform(-100.0, -5.0, batch), rng.uniform(0.0, 20.0, batch)]))
        free = x0 @ cd["Phi"][0].T
        G = cd["Gam"][0]
        qp = batched.PolyQP(cd["H"][0], G, cd["F"][0], p.u_min, p.u_max)
        args = (x0, None, t(np.tile(p.x_min, N)) - free, t(np.tile(p.x_max, N)) - free)
    n = qp.n
    C = torch.cat([G, torch.eye(n, dtype=G.dtype, device=dev)]) if qp.nbox else G
    return qp, args, batched.unpack_lower(cd["H"][0], n), C, cd["F"][0]


MODE = {"solve": "batched"}


def _solve(K, rhs, chunk):
    """torch.linalg.solve in chunks of ``chunk`` systems.  The batched LU of the
    BLAS library works in a workspace of fixed size and refuses batches of
    large systems that do not fit it: the systems are then solved one by one
    (MODE records which of the two ran)."""
    if MODE["solve"] == "batched":
        try:
            return torch.cat([torch.linalg.solve(K[i:i + chunk], rhs[i:i + chunk])
                              for i in range(0, K.shape[0], chunk)])
        except RuntimeError:
            MODE["solve"] = "one by one"
    return torch.stack([torch.linalg.solve(K[i], rhs[i]) for i in range(K.shape[0])])


def _torch_vjp(H, C, F, y, gz, gy, chunk=1 << 30):
    """gf, gx0, ghl, ghu from one dense KKT solve per instance."""
    b, mt = y.shape
    n = H.shape[0]
    D = (y != 0).to(y.dtype)
    DC = D[:, :, None] * C[None]
    K = torch.zeros((b, n + mt, n + mt), dtype=y.dtype, device=y.device)
    K[:, :n, :n] = H
    K[:, n:, :n] = DC
    K[:, :n, n:] = DC.transpose(1, 2)
    K[:, n:, n:] = torch.diag_embed(1 - D)
    s = _solve(K, torch.cat([gz, D * gy], dim=1)[:, :, None], chunk)[:, :, 0]
    gf, e = -s[:, :n], s[:, n:] * D
    zero = torch.zeros_like(e)
    return dict(gf=gf, gx0=gf @ F, ghl=torch.where(y < 0, e, zero), ghu=torch.where(y > 0, e, zero))


def _raw_vjp(qp, y, st, gz, gy):
    """The C entry point on preallocated outputs and scratch."""
    b = y.shape[0]
    o = dict(gf=torch.empty((b, qp.n), dtype=y.dtype, device=y.device),
             gx0=torch.empty((b, qp.nx), dtype=y.dtype, device=y.device),
             ghl=torch.empty_like(y), ghu=torch.empty_like(y), vstatus=torch.empty_like(st))
    scratch = torch.empty((poly_diff.scratch_bytes(qp, b),), dtype=torch.uint8, device=y.device)
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    args = (nat.F64, b, qp.n, qp.m, qp.nbox, qp.nx, qp.ws.data_ptr(), y.data_ptr(), st.data_ptr(),
            None if gz is None else gz.data_ptr(), gy.data_ptr(), *(o[k].data_ptr() for k in OUTS),
            o["vstatus"].data_ptr(), scratch.data_ptr(), scratch.numel(), stream)

    def call():
        nat.check(lib.mpcqp_poly_solve_vjp(*args), "mpcqp_poly_solve_vjp")
    return call, o, scratch


def _step(a):
    dev = torch.device("cuda:0")
    batch = min(a.batch, a.torch_batch) if a.step == "torch" else a.batch
    qp, sargs, H, C, F = _problem(a.shape, batch, dev)
    z, y, st = qp.solve(*sargs)
    ok = batched.status_code(st) == 0
    gen = torch.Generator(device=dev).manual_seed(4)
    gz = torch.randn(z.shape, dtype=z.dtype, device=dev, generator=gen)
    gy = torch.randn(y.shape, dtype=y.dtype, device=dev, generator=gen)
    res = dict(step=a.step, batch=batch, n=qp.n, m_total=qp.mt, nx=qp.nx,
               forward_optimal=int(ok.sum().item()),
               active_rows_mean=(y[ok] != 0).double().sum(1).mean().item())
    if a.step == "vjp":
        r = poly_diff.poly_solve_vjp(qp, y, gz, gy, status=st)
        res["vstatus_optimal"] = int((r["vstatus"] == 0).sum().item())
        k = min(batch, 64)
        good = (r["vstatus"][:k] == 0)[:, None]
        ref = _torch_vjp(H, C, F, torch.where(good, y[:k], torch.zeros_like(y[:k])), gz[:k], gy[:k])
        res["max_abs_diff_vs_torch"] = max(
            (torch.where(good, r[q][:k] - ref[q], torch.zeros_like(ref[q]))).abs().max().item()
            for q in OUTS)
        call, o, _ = _raw_vjp(qp, y, st, gz, gy)
        res["together"] = _median_ms(call, a.warmup, a.repeats)
        assert all(torch.equal(o[q], r[q]) for q in (*OUTS, "vstatus"))
        res.update(_kernel_ms(call, a.repeats))
        res["wrapper"] = _median_ms(lambda: poly_diff.poly_solve_vjp(qp, y, gz, gy, status=st),
                                    a.warmup, a.repeats)
    elif a.step == "forward":
        out = (torch.empty_like(z), torch.empty_like(y), torch.empty_like(st))
        res.update(_median_ms(lambda: qp.solve(*sargs, out=out), a.warmup, a.repeats))
    else:
        y = torch.where(ok[:, None], y, torch.zeros_like(y))   # a failed forward wrote NaN
        res.update(_median_ms(lambda: _torch_vjp(H, C, F, y, gz, gy, a.torch_chunk), a.warmup,
                              a.repeats))
        res["us_per_instance"] = 1e3 * res["median_ms"] / batch
        res["solve_mode"] = MODE["solve"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-batch", type=int, default=1024)
    ap.add_argument("--torch-chunk", type=int, default=64, help="systems per linalg.solve call")
    ap.add_argument("--step-timeout", type=float, default=150.0, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step (child process)")
    ap.add_argument("--shape", choices=tuple(SHAPES), default=None)
    ap.add_argument("--batch", type=int, default=0, help="override the shape's batch")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "poly_vjp", "rate.json"))
    a = ap.parse_args()
    assert a.repeats >= 10
    if a.step:
        a.batch = a.batch or SHAPES[a.shape]
        return _step(a)
    res = dict(what="poly_vjp_rate", dtype="float64", repeats=a.repeats)
    for shape in ((a.shape,) if a.shape else tuple(SHAPES)):
        res[shape] = {}
        for s in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--shape", shape,
                   "--batch", str(a.batch or SHAPES[shape]), "--warmup", str(a.warmup),
                   "--repeats", str(a.repeats), "--torch-batch", str(a.torch_batch),
                   "--torch-chunk", str(a.torch_chunk)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{shape}: step {s} ended with status {p.returncode}")
            res[shape][s] = json.loads(p.stdout.strip().splitlines()[-1])
        r = res[shape]
        r["vjp_over_forward"] = r["vjp"]["together"]["median_ms"] / r["forward"]["median_ms"]
        r["torch_over_vjp_per_instance"] = (r["torch"]["us_per_instance"] * r["vjp"]["batch"]
                                            / (1e3 * r["vjp"]["together"]["median_ms"]))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
