"""Time of the box-MPC loop's adjoint kernel (mpcqp_mpc_box_loop_vjp) at the
2loop shape, next to the forward loop and next to the same gradients as they
could be had without it.

  python tools/box_loop_vjp_rate.py [--batch 4096] [--horizon 20] [--steps 50]
                                    [--repeats 20] [--json profiles/box_loop_vjp/rate.json]

The problem is the 2loop line of bench.py: the FHC double integrator (ts = 0.5,
|u| <= 1, N = 20, fp64), per-instance H, F, A, B, x0 uniform in [-10, 10]^2 from
bench.py's seed, a closed loop of T = 50 steps run once outside the timed region
(xs, zs, status).  The upstream gradients gxs, gus, gzs are standard normal.
Three steps, each a child process of its own under its own time limit (a step
that fails or runs out of time ends the run), each timed with HIP events around
one call, warm-up first, the median of --repeats calls:

  vjp       mpcqp_mpc_box_loop_vjp, every output (gx0, gH, gF, gA, gB, glb, gub,
            gg, gw, vstatus), into buffers allocated beforehand;
  forward   mpcqp_mpc_box_loop with plans on the same batch, into buffers
            allocated beforehand;
  per_step  the same gradients the only way there was before: T times, in
            reverse, mpcqp_solve_box_vjp (the C entry point, on preallocated
            buffers, gf written straight into gg[t]) and the torch ops for
            gz = gzs[t] (+ gus[t] + B'lam), lam <- gxs[t] + A'lam + F'd and the
            outer-product sums into gH, gF, gA, gB, glb, gub, eager.

No threshold is asserted here; the ratios vjp / per_step and vjp / forward are
reported.  Prints one JSON line and writes it to --json.
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

STEPS = ("vjp", "forward", "per_step")
OUTS = batched.LOOP_VJP_OUTPUTS


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
    b, N, T = a.batch, a.horizon, a.steps
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)  # noqa: E731
    rng = np.random.default_rng(20261015 + 2)
    p = dict(A=t(np.broadcast_to(A, (b, 2, 2))), B=t(np.broadcast_to(B, (b, 2, 1))),
             x0=t(rng.uniform(-10.0, 10.0, size=(b, 2))),
             lb=torch.full((N,), -1.0, dtype=torch.float64, device=dev),
             ub=torch.full((N,), 1.0, dtype=torch.float64, device=dev))
    cd = batched.condense(p["A"], p["B"], t(Q), t(np.array([[0.1]])), t(Q), N, outputs=("H", "F"))
    p["H"], p["F"] = cd["H"], cd["F"]
    o = batched.mpc_box_loop(p["A"], p["B"], None, None, None, N, p["x0"], p["lb"], p["ub"], T,
                             plans=True, condensed=cd)
    assert (batched.status_code(o["status"]) == 0).all()
    p.update(xs=o["xs"], us=o["us"], zs=o["zs"], status=o["status"],
             gxs=t(rng.standard_normal((T + 1, b, 2))), gus=t(rng.standard_normal((T, b, 1))),
             gzs=t(rng.standard_normal((T, b, N))))
    return p


def _buffers(p):
    T, b, n = p["zs"].shape
    nx, nu = 2, 1
    shapes = dict(gx0=(b, nx), gH=(b, n * (n + 1) // 2), gF=(b, n, nx), gA=(b, nx, nx),
                  gB=(b, nx, nu), glb=(b, n), gub=(b, n), gg=(T, b, n), gw=(T, b, nx))
    o = {k: torch.empty(s, dtype=torch.float64, device=p["zs"].device) for k, s in shapes.items()}
    o["vstatus"] = torch.empty((b,), dtype=torch.int32, device=p["zs"].device)
    return o


def _raw_vjp(p):
    """The C entry point on preallocated per-instance outputs (lb, ub shared)."""
    T, b, n = p["zs"].shape
    o = _buffers(p)
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    ptr = lambda k: p[k].data_ptr()  # noqa: E731
    args = (nat.F64, b, 2, 1, n, T, ptr("H"), p["H"].shape[1], ptr("F"), 2 * n, ptr("A"), 4,
            ptr("B"), 2, ptr("lb"), 0, ptr("ub"), 0, ptr("xs"), ptr("zs"), ptr("status"),
            ptr("gxs"), ptr("gus"), ptr("gzs"), *(o[k].data_ptr() for k in OUTS),
            o["vstatus"].data_ptr(), stream)

    def call():
        nat.check(lib.mpcqp_mpc_box_loop_vjp(*args), "mpcqp_mpc_box_loop_vjp")
    return call, o


def _raw_forward(p):
    T, b, n = p["zs"].shape
    o = dict(xs=torch.empty_like(p["xs"]), us=torch.empty_like(p["us"]), zs=torch.empty_like(p["zs"]),
             status=torch.empty_like(p["status"]))
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    ptr = lambda k: p[k].data_ptr()  # noqa: E731
    args = (nat.F64, b, 2, 1, n, T, ptr("H"), p["H"].shape[1], ptr("F"), 2 * n, ptr("A"), 4,
            ptr("B"), 2, ptr("x0"), 2, ptr("lb"), 0, ptr("ub"), 0, o["xs"].data_ptr(),
            o["us"].data_ptr(), o["zs"].data_ptr(), o["status"].data_ptr(), 0, 0.0, stream)

    def call():
        nat.check(lib.mpcqp_mpc_box_loop(*args), "mpcqp_mpc_box_loop")
    return call, o


def _per_step(p):
    """T x (mpcqp_solve_box_vjp + torch ops), on preallocated buffers."""
    T, b, n = p["zs"].shape
    o = _buffers(p)
    tmp = dict(glb=torch.empty_like(o["glb"]), gub=torch.empty_like(o["gub"]),
               gH=torch.empty_like(o["gH"]), vs=torch.empty_like(o["vstatus"]))
    lib, stream = nat.load(), torch.cuda.current_stream().cuda_stream
    H, F, A, B = p["H"], p["F"], p["A"], p["B"]

    def call():
        lam = p["gxs"][T]
        for k in ("gH", "gF", "gA", "gB", "glb", "gub"):
            o[k].zero_()
        o["vstatus"].zero_()
        for t in range(T - 1, -1, -1):
            gz = p["gzs"][t].clone()
            gz[:, :1] += p["gus"][t] + torch.einsum("bij,bi->bj", B, lam)
            nat.check(lib.mpcqp_solve_box_vjp(
                nat.F64, b, n, H.data_ptr(), H.shape[1], p["zs"][t].data_ptr(), p["lb"].data_ptr(), 0,
                p["ub"].data_ptr(), 0, p["status"][t].data_ptr(), gz.data_ptr(), o["gg"][t].data_ptr(),
                tmp["glb"].data_ptr(), tmp["gub"].data_ptr(), tmp["gH"].data_ptr(),
                tmp["vs"].data_ptr(), stream), "mpcqp_solve_box_vjp")
            d, x = o["gg"][t], p["xs"][t]
            o["gw"][t] = lam
            o["gH"] += tmp["gH"]
            o["glb"] += tmp["glb"]
            o["gub"] += tmp["gub"]
            o["gF"] += d[:, :, None] * x[:, None, :]
            o["gA"] += lam[:, :, None] * x[:, None, :]
            o["gB"] += lam[:, :, None] * p["zs"][t][:, None, :1]
            torch.maximum(o["vstatus"], tmp["vs"], out=o["vstatus"])
            lam = p["gxs"][t] + torch.einsum("bij,bi->bj", A, lam) + torch.einsum("bij,bi->bj", F, d)
        o["gx0"].copy_(lam)
    return call, o


def _step(a):
    dev = torch.device("cuda:0")
    p = _problem(a, dev)
    on = (p["zs"] == p["lb"]) | (p["zs"] == p["ub"])
    res = dict(step=a.step, active_rows_mean=on.double().sum(2).mean().item())
    if a.step == "vjp":
        call, o = _raw_vjp(p)
        res.update(_median_ms(call, a.warmup, a.repeats))
        assert (o["vstatus"] == 0).all()
        ref_call, ref = _per_step(p)
        ref_call()
        torch.cuda.synchronize()
        res["max_rel_diff_vs_per_step"] = max(
            ((o[k] - ref[k]).abs().max() / (1 + ref[k].abs().max())).item() for k in OUTS)
    elif a.step == "forward":
        call, o = _raw_forward(p)
        res.update(_median_ms(call, a.warmup, a.repeats))
        assert torch.equal(o["zs"], p["zs"])
        res["sweeps_and_iterations_per_step"] = batched.status_iters(p["status"]).double().mean().item()
    else:
        call, _ = _per_step(p)
        res.update(_median_ms(call, a.warmup, a.repeats))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds per step")
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step (child process)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "box_loop_vjp", "rate.json"))
    a = ap.parse_args()
    assert a.horizon <= 32 and a.repeats >= 10 and a.steps >= 1
    if a.step:
        return _step(a)
    res = dict(what="box_loop_vjp_rate", batch=a.batch, n=a.horizon, steps=a.steps, dtype="float64",
               repeats=a.repeats)
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--batch", str(a.batch),
               "--horizon", str(a.horizon), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"step {s} ended with status {p.returncode}")
        res[s] = json.loads(p.stdout.strip().splitlines()[-1])
    res["vjp_over_per_step"] = res["vjp"]["median_ms"] / res["per_step"]["median_ms"]
    res["vjp_over_forward"] = res["vjp"]["median_ms"] / res["forward"]["median_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
