"""Closed-loop rate of the input-box MPC with a per-step linear term and a plant
disturbance: the one-launch device loop (mpcqp_mpc_box_loop_affine) against the
plain loop it extends (mpcqp_mpc_box_loop) and against what exists without it.

  python tools/box_loop_rate.py [--batch 4096] [--steps 50] [--horizon 20]
                                [--repeats 20] [--rounds 5] [--ab-lib OTHER.so]
                                [--no-alternatives] [--json PATH]

The problem is the 2loop line of bench.py: the FHC double integrator (ts = 0.5,
|u| <= 1, N = 20, fp64), per-instance (A, B) and hence per-instance H and F,
x0 uniform in [-10, 10]^2, condensed once outside the timed region.  The
reference is a ramp on the position that levels off, through
batched.tracking_terms.  Times are HIP events around each call, warm-up first,
the median of --repeats launches; for (a) that is repeated in --rounds rounds,
this build and --ab-lib alternately, so that the two builds can be compared
against each build's own round-to-round spread.

  (a) the plain loop of this build and, with --ab-lib, of another build (the
      parent commit's library);
  (b) the affine loop with a g shared by the batch (steps x n);
  (c) the same values as a per-instance g (steps x batch x n);
  (d) per-instance g and a disturbance w (steps x batch x nx);
  (e) today's alternatives on the same tracking problem: the poly loop
      (mpcqp_mpc_poly_loop_affine with m = 0, nbox = 1, one shared plant) and
      the per-step path, T x (f = F x_t + g_t by mpcqp_gemv, mpcqp_solve_box,
      the torch plant) captured in one HIP graph.

MPCQP_LIB selects the library "this" refers to (a -D variant of the kernel, for
instance).  Prints one JSON line (and appends it to --json).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from model_predictive_control_amd import _native as nat  # noqa: E402
from model_predictive_control_amd import batched  # noqa: E402


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _fhc():
    ts = 0.5                                        # FHC.py:44-48, config 2
    A = np.array([[1.0, ts], [0.0, 1.0]])
    B = np.array([[0.0], [-ts]])
    C = np.array([[1.0], [-2.0 / 3.0]])
    Q = C @ C.T + 1e-3 * np.eye(2)
    return A, B, Q, np.array([[0.1]]), Q.copy()


def _outs(b, T, nx, nu, dev):
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(xs=torch.empty((T + 1, b, nx), **f64), us=torch.empty((T, b, nu), **f64),
                status=torch.empty((T, b), dtype=torch.int32, device=dev))


def _stats(o):
    st = o["status"]
    it = ((st >> 8) & 0xFFFF).double()
    return dict(iters_mean=it[1:].mean().item(),
                optimal_fraction=((st & 0xFF) == 0).double().mean().item(),
                saturated_fraction=(o["us"].abs() == 1.0).double().mean().item())


def _equal(a, b, keys=("xs", "us", "status")):
    return all(np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), equal_nan=k != "status")
               for k in keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-alternatives", action="store_true", help="skip (e)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.repeats >= 10
    dev = torch.device("cuda:0")
    b, T, N = a.batch, a.steps, a.horizon
    nx, nu, n = 2, 1, a.horizon
    f64 = dict(dtype=torch.float64, device=dev)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), **f64)  # noqa: E731
    rate = lambda ms: b * T / (ms * 1e-3)  # noqa: E731
    A, B, Q, R, Qf = _fhc()
    Ab, Bb = t(np.broadcast_to(A, (b, 2, 2))), t(np.broadcast_to(B, (b, 2, 1)))
    x0 = t(np.random.default_rng(0).uniform(-10, 10, (b, 2)))
    cd = batched.condense(Ab, Bb, t(Q), t(R), t(Qf), N, outputs=("H", "F", "Gam"))
    H, F = cd["H"], cd["F"]
    lb, ub = torch.full((n,), -1.0, **f64), torch.full((n,), 1.0, **f64)
    res = dict(tool="box_loop_rate", problem=f"fhc_N{N}", batch=b, steps=T, n=n, repeats=a.repeats,
               rounds=a.rounds, lib=os.path.basename(nat.LIB_PATH))
    ptr = batched._ptr
    head = (ptr(H), n * (n + 1) // 2, ptr(F), n * nx, ptr(Ab), nx * nx, ptr(Bb), nx * nu, ptr(x0),
            nx, ptr(lb), 0, ptr(ub), 0)

    # (a) the plain loop: this build, and another build alternately
    libs = {"this": nat.load()}
    if a.ab_lib:
        libs["other"] = ctypes.CDLL(os.path.abspath(a.ab_lib))
    outs = {k: _outs(b, T, nx, nu, dev) for k in libs}

    def plain_call(lib, o):
        fn = lib.mpcqp_mpc_box_loop
        fn.restype, fn.argtypes = nat.SIGNATURES["mpcqp_mpc_box_loop"]
        args = (nat.F64, b, nx, nu, N, T) + head + (ptr(o["xs"]), ptr(o["us"]), None,
                                                    ptr(o["status"]), 0, 0.0, batched._stream())

        def call():
            rc = fn(*args)
            assert rc == 0, rc
        return call

    calls = {k: plain_call(lib, outs[k]) for k, lib in libs.items()}
    med = {k: [] for k in libs}
    for _ in range(a.rounds):
        for k in libs:
            med[k].append(_median_ms(calls[k], a.warmup, a.repeats)[0])
    for k in libs:
        res[f"plain_{k}_round_medians_ms"] = med[k]
        res[f"plain_{k}_ms"] = float(np.median(med[k]))
        res[f"plain_{k}_spread"] = (max(med[k]) - min(med[k])) / float(np.median(med[k]))
        res[f"plain_{k}_steps_per_s"] = rate(res[f"plain_{k}_ms"])
    if a.ab_lib:
        res["plain_outputs_equal"] = _equal(outs["this"], outs["other"])
        res["plain_this_over_other"] = res["plain_this_ms"] / res["plain_other_ms"]
    res["plain"] = _stats(outs["this"])
    plain_ms = res["plain_this_ms"]

    # the reference: a ramp on the position that levels off, velocity 0
    x_ref = torch.zeros((T + N + 1, nx), **f64)
    x_ref[:, 0] = t(np.minimum(0.5 * np.arange(T + N + 1), 8.0))
    g = batched.tracking_terms({"Gam": cd["Gam"][0]}, t(Q), t(R), t(Qf), N, T, x_ref)   # (T, n)
    gb = g[:, None].expand(T, b, n).contiguous()
    w = 0.05 * torch.as_tensor(np.random.default_rng(1).normal(size=(T, b, nx)), **f64)

    def affine_run(gg, ww):
        # a direct call like the plain loop's, so that both are timed alike
        o = _outs(b, T, nx, nu, dev)
        lib = nat.load()
        args = (nat.F64, b, nx, nu, N, T, 0) + head + (
            ptr(gg), 0 if gg is None or gg.ndim == 2 else n, ptr(ww), ptr(o["xs"]), ptr(o["us"]),
            None, ptr(o["status"]), 0, 0.0, batched._stream())

        def fn():
            rc = lib.mpcqp_mpc_box_loop_affine(*args)
            assert rc == 0, rc
        ms, lo, hi = _median_ms(fn, a.warmup, a.repeats)
        return o, dict(ms=ms, min_ms=lo, max_ms=hi, steps_per_s=rate(ms),
                       ms_over_plain=ms / plain_ms, **_stats(o))

    o_sh, res["affine_shared_g"] = affine_run(g, None)                     # (b)
    o_pi, res["affine_per_instance_g"] = affine_run(gb, None)              # (c)
    res["shared_equals_per_instance"] = _equal(o_sh, o_pi)
    _, res["affine_g_and_w"] = affine_run(gb, w)                           # (d)
    res["g_bytes_per_step_and_instance"] = n * 8
    res["g_read_GBps_at_rate_c"] = n * 8 * res["affine_per_instance_g"]["steps_per_s"] / 1e9

    if not a.no_alternatives:
        # (e1) the poly loop on the same problem: no rows, the input box, one shared plant
        r = batched.mpc_poly_loop(t(A), t(B), t(Q), t(R), t(Qf), N, x0, None, None, -1.0, 1.0, T,
                                  x_ref=x_ref)
        torch.cuda.synchronize()
        diff = (r["xs"] - o_sh["xs"]).abs().max().item()
        cdp = r["condensed"]
        qp = batched.PolyQP(cdp["H"], None, cdp["F"], lb, ub)
        op = _outs(b, T, nx, nu, dev)
        op["scratch"] = torch.empty((qp.affine_scratch_bytes(b, T, True),), dtype=torch.uint8,
                                    device=dev)
        At, Bt = t(A), t(B)
        ms = _median_ms(lambda: qp.loop(At, Bt, x0, T, g=g, out=op), a.warmup, a.repeats)[0]
        res["poly_loop_affine"] = dict(ms=ms, steps_per_s=rate(ms), ms_over_plain=ms / plain_ms,
                                       max_abs_x_diff_vs_box_loop=diff,
                                       optimal_fraction=((op["status"] & 0xFF) == 0).double()
                                       .mean().item())

        # (e2) the per-step path, T steps in one HIP graph
        xs = torch.empty((T + 1, b, nx), **f64)
        zs = torch.empty((T, b, n), **f64)
        f = torch.empty((b, n), **f64)
        st = torch.empty((T, b), dtype=torch.int32, device=dev)
        AT, BT = At.T.contiguous(), Bt.T.contiguous()
        tmp = torch.empty((b, nx), **f64)

        def episode():
            xs[0].copy_(x0)
            for k in range(T):
                f.copy_(gb[k])
                batched.gemv(F, xs[k], 1.0, 1.0, f)
                batched.solve_box(H, f, lb, ub, out=(zs[k], st[k]))
                torch.mm(xs[k], AT, out=tmp)
                torch.addmm(tmp, zs[k, :, :nu], BT, out=xs[k + 1])

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            episode()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            episode()
        ms = _median_ms(graph.replay, a.warmup, a.repeats)[0]
        torch.cuda.synchronize()
        res["per_step_graph"] = dict(ms=ms, steps_per_s=rate(ms), ms_over_plain=ms / plain_ms,
                                     optimal_fraction=((st & 0xFF) == 0).double().mean().item(),
                                     max_abs_x_diff_vs_box_loop=(xs - o_sh["xs"]).abs().max().item())
        res["speedup_per_instance_g_vs_per_step"] = ms / res["affine_per_instance_g"]["ms"]

    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
