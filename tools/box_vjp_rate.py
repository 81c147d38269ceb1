"""Time of the box-QP adjoint kernel (mpcqp_solve_box_vjp) at the config-2
shape, next to what exists without it and next to the forward solve.

  python tools/box_vjp_rate.py [--batch 4096] [--horizon 20] [--repeats 20]
                               [--json profiles/box_vjp/rate.json]

The problem is the cfg2 line of bench.py: the FHC double integrator (ts = 0.5,
|u| <= 1, N = 20, fp64), per-instance H, x0 uniform in [-10, 10]^2 from bench.py's
seed, condensed and solved once outside the timed region.  gz is standard
normal.  Three steps, each a child process of its own under its own time limit
(a step that fails or runs out of time ends the run), each timed with HIP
events around one call, warm-up first, the median of --repeats calls:

  vjp      mpcqp_solve_box_vjp with all four gradients (gf, glb, gub, gH) into
           buffers allocated beforehand, as the forward is timed; next to it
           "wrapper": batched.solve_box_vjp, which also allocates the outputs
           and sums glb / gub of the shared bounds over the batch;
  torch    the same gradients without it: torch.linalg.solve on H with the
           active rows and columns replaced by the identity (d), the H_AF
           product (nu) and the outer products folded onto the packed
           entries (gH), all batched torch ops on the device;
  forward  mpcqp_solve_box on the same batch.

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
from model_predictive_control_amd import batched  # noqa: E402

STEPS = ("vjp", "torch", "forward")


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


def _problem(a, dev):
    ts = 0.5                                        # FHC.py:44-48, config 2
    A = np.array([[1.0, ts], [0.0, 1.0]])
    B = np.array([[0.0], [-ts]])
    C = np.array([[1.0], [-2.0 / 3.0]])
    Q = C @ C.T + 1e-3 * np.eye(2)
    b, N = a.batch, a.horizon
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)  # noqa: E731
    rng = np.random.default_rng(20261015 + 2)
    X0 = rng.uniform(-10.0, 10.0, size=(b, 2))
    cd = batched.condense(t(np.broadcast_to(A, (b, 2, 2))), t(np.broadcast_to(B, (b, 2, 1))), t(Q),
                          t(np.array([[0.1]])), t(Q), N, x0=t(X0), outputs=("H", "f"))
    lb = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
    ub = torch.full((N,), 1.0, dtype=torch.float64, device=dev)
    z, st = batched.solve_box(cd["H"], cd["f"], lb, ub)
    gz = t(rng.standard_normal((b, N)))
    assert (batched.status_code(st) == 0).all()
    return cd["H"], cd["f"], lb, ub, z, st, gz


def _torch_vjp(H, z, lb, ub, gz):
    """The gradients of solve_box_vjp from batched torch ops alone."""
    n = z.shape[1]
    Hd = batched.unpack_lower(H, n)
    at_lb = z == lb
    at_ub = (z == ub) & ~at_lb
    act = at_lb | at_ub
    free = (~act).to(z.dtype)
    eye = torch.eye(n, dtype=z.dtype, device=z.device)
    Hm = Hd * free[:, :, None] * free[:, None, :] + eye * act.to(z.dtype)[:, None, :]
    d = -torch.linalg.solve(Hm, (gz * free)[:, :, None])[:, :, 0] * free
    nu = torch.where(act, gz + torch.einsum("bij,bj->bi", Hd, d), torch.zeros_like(gz))
    G = d[:, :, None] * z[:, None, :]
    G = G + G.transpose(1, 2) - torch.diag_embed(torch.diagonal(G, dim1=1, dim2=2))
    return dict(gf=d, glb=torch.where(at_lb, nu, torch.zeros_like(nu)),
                gub=torch.where(at_ub, nu, torch.zeros_like(nu)), gH=batched.pack_lower(G))


def _raw_vjp(H, z, lb, ub, gz, st):
    """The C entry point on preallocated per-instance outputs (lb, ub shared)."""
    b, n = z.shape
    o = dict(gf=torch.empty_like(z), glb=torch.empty_like(z), gub=torch.empty_like(z),
             gH=torch.empty_like(H), vstatus=torch.empty_like(st))
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in o.items()}
    args = (nat.F64, b, n, H.data_ptr(), H.shape[1], z.data_ptr(), lb.data_ptr(), 0, ub.data_ptr(),
            0, st.data_ptr(), gz.data_ptr(), ptr["gf"], ptr["glb"], ptr["gub"], ptr["gH"],
            ptr["vstatus"], stream)

    def call():
        nat.check(lib.mpcqp_solve_box_vjp(*args), "mpcqp_solve_box_vjp")
    return call, o


def _step(a):
    dev = torch.device("cuda:0")
    H, f, lb, ub, z, st, gz = _problem(a, dev)
    on = (z == lb) | (z == ub)
    res = dict(step=a.step, active_rows_mean=on.double().sum(1).mean().item())
    if a.step == "vjp":
        r = batched.solve_box_vjp(H, z, lb, ub, gz, status=st)
        assert (r["vstatus"] == 0).all()
        ref = _torch_vjp(H, z, lb, ub, gz)
        res["max_abs_diff_vs_torch"] = max(
            (r["gf"] - ref["gf"]).abs().max().item(), (r["glb"] - ref["glb"].sum(0)).abs().max().item(),
            (r["gub"] - ref["gub"].sum(0)).abs().max().item(), (r["gH"] - ref["gH"]).abs().max().item())
        call, o = _raw_vjp(H, z, lb, ub, gz, st)
        res.update(_median_ms(call, a.warmup, a.repeats))
        assert all(torch.equal(o[k], r[k]) for k in ("gf", "gH", "vstatus"))
        res["wrapper"] = _median_ms(lambda: batched.solve_box_vjp(H, z, lb, ub, gz, status=st),
                                    a.warmup, a.repeats)
    elif a.step == "torch":
        res.update(_median_ms(lambda: _torch_vjp(H, z, lb, ub, gz), a.warmup, a.repeats))
    else:
        out = (torch.empty_like(z), torch.empty_like(st))
        res.update(_median_ms(lambda: batched.solve_box(H, f, lb, ub, out=out), a.warmup, a.repeats))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step (child process)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "box_vjp", "rate.json"))
    a = ap.parse_args()
    assert a.horizon <= 32 and a.repeats >= 10
    if a.step:
        return _step(a)
    res = dict(what="box_vjp_rate", batch=a.batch, n=a.horizon, dtype="float64", repeats=a.repeats)
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--batch", str(a.batch),
               "--horizon", str(a.horizon), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"step {s} ended with status {p.returncode}")
        res[s] = json.loads(p.stdout.strip().splitlines()[-1])
    res["vjp_over_forward"] = res["vjp"]["median_ms"] / res["forward"]["median_ms"]
    res["torch_over_vjp"] = res["torch"]["median_ms"] / res["vjp"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
