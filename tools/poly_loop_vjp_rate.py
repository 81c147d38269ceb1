"""Time of the adjoint of the one-launch state-constrained MPC loop
(mpcqp_mpc_poly_loop_vjp) against the forward loop it differentiates and
against the path that exists without it -- T x (mpcqp_poly_solve_vjp + the torch
operations of the reverse-time recursion), captured in one HIP graph.

  python tools/poly_loop_vjp_rate.py [--batch 4096] [--steps 50] [--repeats 20]
                                     [--json profiles/poly_loop_vjp/rate.json]

Both shapes of tools/poly_loop_rate.py (its problem builders are used): the
session-2 Problem at N = 5 and BASELINE config 4 (n = 200, 40 rows), fp64.
Times are HIP events around each path, warm-up first, median of the repeats.
Per shape:
  forward           PolyQP.loop with plans and multipliers (what the adjoint reads)
  forward_bare      PolyQP.loop without them (the line of poly_loop_rate.py)
  vjp_no_gzs        a loss on xs and us: one launch, no scratch, every output
  vjp_no_gzs_no_gf  the same without gf: no n-wide work
  vjp_gzs           all four upstreams: the product launch, then the adjoint
  per_step_graph    the per-step path with all four upstreams
and the mean number of active rows per step (= sweeps per step of the adjoint)
and the largest difference of gx0 between the one-launch and the per-step path
over the instances both call OPTIMAL.  Writes one JSON document with both
shapes to --json and prints it.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from model_predictive_control_amd import poly_diff  # noqa: E402
from poly_loop_rate import _config4, _median_ms, _session2  # noqa: E402


def measure(p, T, warmup, repeats, dev):
    qp, A, B, x0, hl, hu, E = (p[k] for k in ("qp", "A", "B", "x0", "hl", "hu", "E"))
    b, nx, nu, n, m, mt = x0.shape[0], A.shape[0], B.shape[1], qp.n, qp.m, qp.mt
    f64 = dict(dtype=torch.float64, device=dev)
    res = dict(problem=p["name"], batch=b, steps=T, n=n, m_total=mt, bs=(mt + 7) // 8)

    o = qp.loop(A, B, x0, T, hl, hu, E, plans=True, multipliers=True)
    bare = qp.loop(A, B, x0, T, hl, hu, E)
    ms = lambda fn: _median_ms(fn, warmup, repeats)[0]  # noqa: E731
    res["forward_ms"] = ms(lambda: qp.loop(A, B, x0, T, hl, hu, E, plans=True, multipliers=True,
                                           out=o))
    res["forward_bare_ms"] = ms(lambda: qp.loop(A, B, x0, T, hl, hu, E, out=bare))
    ys, st = o["ys"], o["status"]
    code = st & 0xFF
    res["optimal_instances"] = (code == 0).all(dim=0).double().mean().item()
    live = (code == 0).all(dim=0)
    res["active_rows_per_step_mean"] = (ys[:, live] != 0).sum(-1).double().mean().item()
    res["active_rows_per_step_max"] = int((ys[:, live] != 0).sum(-1).max().item())

    gen = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dev)  # noqa: E731
    gxs, gus, gzs, gys = rnd(T + 1, b, nx), rnd(T, b, nu), rnd(T, b, n), rnd(T, b, mt)
    scratch = torch.empty((poly_diff.loop_scratch_bytes(qp, b, T),), dtype=torch.uint8, device=dev)
    every = poly_diff.LOOP_VJP_OUTPUTS
    no_gf = tuple(k for k in every if k != "gf")

    def vjp(ups, need, scr=None):
        return poly_diff.poly_loop_vjp(qp, A, B, ys, *ups, E=E, status=st, need=need, scratch=scr)

    res["vjp_no_gzs_ms"] = ms(lambda: vjp((gxs, gus, None, None), every))
    res["vjp_no_gzs_no_gf_ms"] = ms(lambda: vjp((gxs, gus, None, None), no_gf))
    res["vjp_gzs_ms"] = ms(lambda: vjp((gxs, gus, gzs, gys), every, scratch))
    one = vjp((gxs, gus, gzs, gys), every, scratch)

    # the per-step path: T x (mpcqp_poly_solve_vjp + the recursion in torch), one graph
    step_scratch = torch.empty((poly_diff.scratch_bytes(qp, b),), dtype=torch.uint8, device=dev)
    gw = torch.empty((T, b, nx), **f64)
    gf = torch.empty((T, b, n), **f64)
    ghl, ghu = torch.empty((b, mt), **f64), torch.empty((b, mt), **f64)
    gx0 = torch.empty((b, nx), **f64)
    vs = torch.empty((T, b), dtype=torch.int32, device=dev)

    def episode():
        lam = gxs[T]
        ghl.zero_()
        ghu.zero_()
        for t in range(T - 1, -1, -1):
            gz = gzs[t].clone()
            gz[:, :nu] += gus[t] + lam @ B
            r = poly_diff.poly_solve_vjp(qp, ys[t], gz, gys[t], status=st[t], scratch=step_scratch)
            gw[t].copy_(lam)
            gf[t].copy_(r["gf"])
            vs[t].copy_(r["vstatus"])
            ghl.add_(r["ghl"])
            ghu.add_(r["ghu"])
            lam = gxs[t] + lam @ A + r["gx0"]
            if E is not None:
                lam = lam - r["e"][:, :m] @ E
        gx0.copy_(lam)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        episode()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        episode()
    res["per_step_graph_ms"] = ms(graph.replay)
    torch.cuda.synchronize()
    both = (one["vstatus"] == 0) & (vs == 0).all(dim=0)
    res["vjp_optimal_instances"] = (one["vstatus"] == 0).double().mean().item()
    res["max_abs_gx0_diff_vs_per_step"] = (one["gx0"][both] - gx0[both]).abs().max().item()
    res["max_abs_gx0"] = one["gx0"][both].abs().max().item()
    res["speedup_vjp_gzs_vs_per_step"] = res["per_step_graph_ms"] / res["vjp_gzs_ms"]
    res["vjp_no_gzs_over_forward"] = res["vjp_no_gzs_ms"] / res["forward_ms"]
    res["vjp_gzs_over_forward"] = res["vjp_gzs_ms"] / res["forward_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "poly_loop_vjp", "rate.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = dict(tool="poly_loop_vjp_rate", dtype="float64", repeats=a.repeats, warmup=a.warmup,
               device=torch.cuda.get_device_name(0),
               shapes=[measure(build(a.batch, dev), a.steps, a.warmup, a.repeats, dev)
                       for build in (_session2, _config4)])
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
