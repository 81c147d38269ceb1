"""Time of the adjoint kernel of condensing (mpcqp_condense_vjp) next to what
exists without it and next to the forward condensing.

  python tools/condense_vjp_rate.py [--batch 4096] [--repeats 20]
                                    [--json profiles/condense_vjp/rate.json]

Two shapes, fp64, time-invariant per-instance plants of spectral radius <= 1
with per-instance SPD weights, c and x0 (nothing shared, so no gradient is
summed over the batch): the 2loop shape (nx, nu, N) = (2, 1, 20) and (4, 2, 16).
The upstream gradients gH, gF, gf are standard normal.  Three steps per shape,
each a child process of its own under its own time limit (a step that fails or
runs out of time ends the run), each timed with HIP events around one call,
warm-up first, the median of --repeats calls:

  vjp      mpcqp_condense_vjp with all seven gradients into buffers allocated
           beforehand; next to it "wrapper": condense_diff.condense_vjp, which
           also allocates the outputs;
  torch    the same gradients without it: torch.autograd.grad of
           <gH, H> + <gF, F> + <gf, f> through a restatement of condensing in
           batched torch ops on the device (forward and backward timed together:
           the adjoint kernel runs its own forward pass too);
  forward  mpcqp_condense (H, F, f) on the same batch.

The vjp step also reports the largest difference between the kernel's and
torch's gradients.  The condition is torch_over_vjp >= 1 at both shapes.
Prints one JSON line and writes it to --json.
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
from model_predictive_control_amd.condense_diff import VJP_OUTPUTS, condense_vjp  # noqa: E402

STEPS = ("vjp", "torch", "forward")
SHAPES = ((2, 1, 20), (4, 2, 16))
INPUTS = ("A", "B", "Q", "R", "Qf", "c", "x0")


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


def _problem(b, nx, nu, N, dev):
    rng = np.random.default_rng(20261021 + 100 * nx + 10 * nu + N)
    n = N * nu
    A = rng.standard_normal((b, nx, nx))
    A *= (rng.uniform(0.6, 1.0, b) / np.abs(np.linalg.eigvals(A)).max(axis=-1))[:, None, None]

    def spd(k):
        M = rng.standard_normal((b, k, k))
        return M @ np.swapaxes(M, -1, -2) / k + 0.5 * np.eye(k)

    p = dict(A=A, B=rng.standard_normal((b, nx, nu)), Q=spd(nx), R=spd(nu), Qf=spd(nx),
             c=rng.standard_normal((b, N, nx)), x0=rng.standard_normal((b, nx)),
             gH=rng.standard_normal((b, n * (n + 1) // 2)), gF=rng.standard_normal((b, n, nx)),
             gf=rng.standard_normal((b, n)))
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)
            for k, v in p.items()}


def _torch_condense(A, B, Q, R, Qf, c, x0, N):
    """H (packed), F, f of batched.condense from batched torch ops."""
    b, nx, nu = B.shape
    n = N * nu
    G = A.new_zeros((b, nx, n))
    P = torch.eye(nx, dtype=A.dtype, device=A.device).expand(b, nx, nx)
    x = x0
    H = torch.einsum("kl,bij->bkilj", torch.eye(N, dtype=A.dtype, device=A.device), R).reshape(b, n, n)
    F = A.new_zeros((b, n, nx))
    f = A.new_zeros((b, n))
    for k in range(N):
        G = A @ G
        G = torch.cat([G[:, :, :k * nu], B, G[:, :, (k + 1) * nu:]], dim=2)
        P = A @ P
        x = torch.einsum("bij,bj->bi", A, x) + c[:, k]
        GQ = G.transpose(1, 2) @ (Qf if k == N - 1 else Q)
        H = H + GQ @ G
        F = F + GQ @ P
        f = f + torch.einsum("bij,bj->bi", GQ, x)
    return batched.pack_lower(H), F, f


def _torch_vjp(t, N):
    a = [t[k].detach().requires_grad_(True) for k in INPUTS]
    H, F, f = _torch_condense(*a, N)
    L = (t["gH"] * H).sum() + (t["gF"] * F).sum() + (t["gf"] * f).sum()
    g = dict(zip(("gA", "gB", "gQ", "gR", "gQf", "gc", "gx0"), torch.autograd.grad(L, a)))
    for k in ("gQ", "gR", "gQf"):
        g[k] = 0.5 * (g[k] + g[k].transpose(1, 2))
    return g


def _raw_vjp(t, nx, nu, N):
    """The C entry point on preallocated per-instance outputs."""
    b = t["A"].shape[0]
    shapes = dict(gA=(b, nx, nx), gB=(b, nx, nu), gQ=(b, nx, nx), gR=(b, nu, nu), gQf=(b, nx, nx),
                  gc=(b, N, nx), gx0=(b, nx))
    o = {k: torch.empty(s, dtype=torch.float64, device=t["A"].device) for k, s in shapes.items()}
    o["vstatus"] = torch.empty((b,), dtype=torch.int32, device=t["A"].device)
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    head = []
    for k in INPUTS:
        head += [t[k].data_ptr(), int(t[k][0].numel())]
    args = (nat.F64, b, nx, nu, N, 0, *head, t["gH"].data_ptr(), t["gF"].data_ptr(),
            t["gf"].data_ptr(), *(o[k].data_ptr() for k in VJP_OUTPUTS), o["vstatus"].data_ptr(),
            stream)

    def call():
        nat.check(lib.mpcqp_condense_vjp(*args), "mpcqp_condense_vjp")
    return call, o


def _step(a):
    dev = torch.device("cuda:0")
    nx, nu, N = a.shape
    t = _problem(a.batch, nx, nu, N, dev)
    res = dict(step=a.step, shape=[nx, nu, N])
    plant = [t[k] for k in ("A", "B", "Q", "R", "Qf")]
    if a.step == "vjp":
        call, o = _raw_vjp(t, nx, nu, N)
        call()
        torch.cuda.synchronize()
        assert (o["vstatus"] == 0).all()
        ref = _torch_vjp(t, N)
        res["max_abs_diff_vs_torch"] = max((o[k] - ref[k]).abs().max().item() for k in VJP_OUTPUTS)
        res["max_abs_gradient"] = max(ref[k].abs().max().item() for k in VJP_OUTPUTS)
        res.update(_median_ms(call, a.warmup, a.repeats))
        res["wrapper"] = _median_ms(
            lambda: condense_vjp(*plant, N, t["x0"], t["c"], gH=t["gH"], gF=t["gF"], gf=t["gf"]),
            a.warmup, a.repeats)
    elif a.step == "torch":
        res.update(_median_ms(lambda: _torch_vjp(t, N), a.warmup, a.repeats))
    else:
        out = batched.condense(*plant, N, x0=t["x0"], c=t["c"], outputs=("H", "F", "f"))
        res.update(_median_ms(lambda: batched.condense(*plant, N, x0=t["x0"], c=t["c"],
                                                       outputs=("H", "F", "f"), out=out),
                              a.warmup, a.repeats))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step (child process)")
    ap.add_argument("--shape", type=int, nargs=3, default=None, help="nx nu N of a child's step")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "condense_vjp", "rate.json"))
    a = ap.parse_args()
    assert a.repeats >= 10
    if a.step:
        return _step(a)
    res = dict(what="condense_vjp_rate", batch=a.batch, dtype="float64", repeats=a.repeats, shapes=[])
    for shape in SHAPES:
        r = dict(shape=list(shape))
        for s in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--shape",
                   *map(str, shape), "--batch", str(a.batch), "--warmup", str(a.warmup),
                   "--repeats", str(a.repeats)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"step {s} at {shape} ended with status {p.returncode}")
            r[s] = json.loads(p.stdout.strip().splitlines()[-1])
        r["vjp_over_forward"] = r["vjp"]["median_ms"] / r["forward"]["median_ms"]
        r["torch_over_vjp"] = r["torch"]["median_ms"] / r["vjp"]["median_ms"]
        res["shapes"].append(r)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
