"""Closed-loop rate of the state-constrained linear MPC: the one-launch device
loop (mpcqp_mpc_poly_loop, warm and cold) against the per-step path that
exists without it -- T x (PolyQP.solve with out= + the row-bound update
hl - Phi x_t, hu - Phi x_t + the torch plant), captured in one HIP graph.

  python tools/poly_loop_rate.py [--config4] [--batch 4096] [--steps 50]
                                 [--repeats 20] [--json PATH]

Default: the session-2 Problem (session_2/problem.py:4-33), N = 5, Qf = Q, x0
uniform in p in [-100, 0], v in [-15, 25].  --config4: nx = 12, nu = 4, N = 50,
40 fixed rows on the plan (BASELINE config 4; no row-bound update).  Times are
HIP events around each path, warm-up first, median of the repeats.  Prints one
JSON line (and appends it to --json).

  python tools/poly_loop_rate.py --soft [--config4 | --horizon N] [--ab-lib OTHER.so] ...

--soft measures the soft loop (mpcqp_mpc_poly_loop_soft) instead:
  1. the hard warm loop of this build, and with --ab-lib the same call into
     another build of the library (the parent commit's), timed alternately in
     --rounds rounds of --repeats launches: the median of each round, so that
     the two builds can be compared against each build's own spread;
  2. (session-2 batch only) the soft loop with rho = 2000, sigma = 1 on the
     same batch (the hard loop's iterations wherever the hard QP is feasible)
     and with rho = inf (the hard loop's iterations everywhere): the price of
     the variant;
  3. (session-2 batch only) Problem(u_min=-2.0), x0 drawn the same way: the
     soft loop with (50, 1) -- rate, share of softened steps, iterations --
     and the hard loop on it -- rate, share of dead (instance, step) pairs.

  python tools/poly_loop_rate.py --affine [--config4] [--ab-lib OTHER.so] ...

--affine measures the loop with a per-step linear term (mpcqp_mpc_poly_loop_affine):
  (i)   the hard warm loop of this build and of --ab-lib, alternately, as --soft does;
  (ii)  the new entry point with a g shared by the batch: a ramp reference on
        the first state, through batched.tracking_terms;
  (iii) the same values as a per-instance g (steps x batch x n): the same loop
        iterations, so that (iii) - (ii) is what the batch-sized product -Hinv g,
        -Ut g (the prep kernel) and the per-instance reads cost;
  (iv)  the per-step path with the same term: T x (PolyQP.solve(x, f=g_t, out=)
        + the row-bound update + the torch plant) in one HIP graph.
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
from model_predictive_control_amd.problems import Problem  # noqa: E402


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
    return float(np.median(ts)), float(np.min(ts))


def _session2(batch, dev, pr=None, N=None):
    pr = pr or Problem()
    if N:
        pr.N = N
    t = lambda a: torch.as_tensor(np.asarray(a, float), dtype=torch.float64, device=dev)  # noqa: E731
    N = pr.N
    cd = batched.condense(t(pr.A), t(pr.B), t(pr.Q), t(pr.R), t(pr.Q), N,
                          outputs=("H", "F", "Gam", "Phi"))
    cd = {k: v[0] for k, v in cd.items()}
    n = N * pr.n_input
    qp = batched.PolyQP(cd["H"], cd["Gam"], cd["F"], torch.full((n,), pr.u_min, dtype=torch.float64),
                        torch.full((n,), pr.u_max, dtype=torch.float64), device=dev)
    rng = np.random.default_rng(0)
    x0 = np.stack([rng.uniform(-100, 0, batch), rng.uniform(-15, 25, batch)], axis=1)
    return dict(qp=qp, A=t(pr.A), B=t(pr.B), x0=t(x0), hl=t(np.tile(pr.x_min, N)),
                hu=t(np.tile(pr.x_max, N)), E=cd["Phi"], name=f"session2_N{N}")


def _config4(batch, dev):
    nx, nu, N, m = 12, 4, 50, 40
    rng = np.random.default_rng(nx * 100 + N)
    t = lambda a: torch.as_tensor(np.asarray(a, float), dtype=torch.float64, device=dev)  # noqa: E731
    U, _ = np.linalg.qr(rng.normal(size=(nx, nx)))
    A = (U * rng.uniform(0.5, 0.98, nx)) @ U.T
    B = rng.normal(size=(nx, nu)) / np.sqrt(nx)
    cd = batched.condense(t(A), t(B), t(np.eye(nx)), t(0.1 * np.eye(nu)), t(np.eye(nx)), N,
                          outputs=("H", "F"))
    G = rng.normal(size=(m, N * nu))
    hu = rng.uniform(0.5, 1.5, size=m)
    qp = batched.PolyQP(cd["H"][0], t(G), cd["F"][0])
    x0 = rng.normal(size=(batch, nx)) * 3
    return dict(qp=qp, A=t(A), B=t(B), x0=t(x0), hl=None, hu=t(hu), E=None, name="config4")


def _hard_loop_call(lib, p, T, o):
    """The hard warm loop as a direct call into ``lib`` (this build's library or
    another build's; the workspace layout is that of mpcqp_poly_setup)."""
    qp, A, B, x0, hl, hu, E = (p[k] for k in ("qp", "A", "B", "x0", "hl", "hu", "E"))
    ptr = batched._ptr
    fn = lib.mpcqp_mpc_poly_loop
    fn.restype, fn.argtypes = nat.SIGNATURES["mpcqp_mpc_poly_loop"]
    args = (nat.F64, x0.shape[0], qp.n, qp.m, qp.nbox, A.shape[0], B.shape[1], T, 0, ptr(qp.ws),
            ptr(E), ptr(A), ptr(B), ptr(x0), A.shape[0], ptr(hl), ptr(hu), 0, ptr(qp.lbz),
            ptr(qp.ubz), None, ptr(o["xs"]), ptr(o["us"]), None, None, ptr(o["status"]), 0, 0.0,
            batched._stream())

    def call():
        rc = fn(*args)
        assert rc == 0, rc
    return call


def _outs(b, T, nx, nu, dev):
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(xs=torch.empty((T + 1, b, nx), **f64), us=torch.empty((T, b, nu), **f64),
                status=torch.empty((T, b), dtype=torch.int32, device=dev))


def _stats(o):
    st = o["status"]
    code = st & 0xFF
    it = ((st >> 8) & 0xFFFF).double()
    return dict(iters_mean=it[1:].mean().item(),
                iters_per_episode_max=it.sum(dim=0).max().item(),
                optimal_fraction=(code == 0).double().mean().item(),
                dead_fraction=(code > 1).double().mean().item(),
                softened_fraction=((st & nat.STATUS_SOFTENED) != 0).double().mean().item())


def soft_mode(a, dev):
    b, T = a.batch, a.steps
    rate = lambda ms: b * T / (ms * 1e-3)  # noqa: E731
    p = _config4(b, dev) if a.config4 else _session2(b, dev, N=a.horizon)
    nx, nu = p["A"].shape[0], p["B"].shape[1]
    res = dict(tool="poly_loop_rate", mode="soft", problem=p["name"], batch=b, steps=T,
               m_total=p["qp"].mt, repeats=a.repeats, rounds=a.rounds)

    # 1. the hard warm loop: this build, and another build alternately
    libs = {"this": nat.load()}
    if a.ab_lib:
        libs["other"] = ctypes.CDLL(os.path.abspath(a.ab_lib))
    outs = {k: _outs(b, T, nx, nu, dev) for k in libs}
    calls = {k: _hard_loop_call(lib, p, T, outs[k]) for k, lib in libs.items()}
    med = {k: [] for k in libs}
    for _ in range(a.rounds):
        for k in libs:
            med[k].append(_median_ms(calls[k], a.warmup, a.repeats)[0])
    for k in libs:
        res[f"hard_{k}_round_medians_ms"] = med[k]
        res[f"hard_{k}_ms"] = float(np.median(med[k]))
        res[f"hard_{k}_steps_per_s"] = rate(float(np.median(med[k])))
    if a.ab_lib:
        res["hard_outputs_equal"] = all(torch.equal(outs["this"][k], outs["other"][k])
                                        if k == "status" else
                                        torch.equal(outs["this"][k].isnan(), outs["other"][k].isnan())
                                        and bool((outs["this"][k].nan_to_num() ==
                                                  outs["other"][k].nan_to_num()).all())
                                        for k in ("xs", "us", "status"))
    res["hard"] = _stats(outs["this"])

    if not a.config4:
        def soft_run(pp, rho, sigma):
            # a direct call like the hard loop's, so that both are timed alike
            o = _outs(b, T, nx, nu, dev)
            qq, m = pp["qp"], pp["qp"].m
            pen = (torch.full((m,), rho, dtype=torch.float64, device=dev),
                   torch.full((m,), sigma, dtype=torch.float64, device=dev))
            ptr = batched._ptr
            lib = nat.load()
            args = (nat.F64, b, qq.n, m, qq.nbox, nx, nu, T, 0, ptr(qq.ws), ptr(pp["E"]),
                    ptr(pp["A"]), ptr(pp["B"]), ptr(pp["x0"]), nx, ptr(pp["hl"]), ptr(pp["hu"]), 0,
                    ptr(qq.lbz), ptr(qq.ubz), None, ptr(pen[0]), ptr(pen[1]), ptr(o["xs"]),
                    ptr(o["us"]), None, None, None, ptr(o["status"]), 0, 0.0, batched._stream())

            def fn():
                rc = lib.mpcqp_mpc_poly_loop_soft(*args)
                assert rc == 0, rc
            ms = _median_ms(fn, a.warmup, a.repeats)[0]
            return dict(ms=ms, steps_per_s=rate(ms), **_stats(o))

        # 2. the price of the variant: same batch, same iterations
        s2 = soft_run(p, 2000.0, 1.0)
        s2["ms_over_hard"] = s2["ms"] / res["hard_this_ms"]
        res["soft_rho2000"] = s2
        # ... and with every row hard (rho = inf): the hard loop's very trips
        s0 = soft_run(p, float("inf"), 1.0)
        s0["ms_over_hard"] = s0["ms"] / res["hard_this_ms"]
        res["soft_rho_inf"] = s0
        # 3. a batch that loses feasibility
        q = _session2(b, dev, Problem(u_min=-2.0), N=a.horizon)
        oh = _outs(b, T, nx, nu, dev)
        ms_h = _median_ms(_hard_loop_call(nat.load(), q, T, oh), a.warmup, a.repeats)[0]
        res["umin2_hard"] = dict(ms=ms_h, steps_per_s=rate(ms_h), **_stats(oh))
        res["umin2_soft_50_1"] = soft_run(q, 50.0, 1.0)
    return res


def _ab_hard(a, p, T, dev, res):
    """The hard warm loop of this build and, with --ab-lib, of another build,
    timed alternately: the median of each round."""
    b, nx, nu = a.batch, p["A"].shape[0], p["B"].shape[1]
    libs = {"this": nat.load()}
    if a.ab_lib:
        libs["other"] = ctypes.CDLL(os.path.abspath(a.ab_lib))
    outs = {k: _outs(b, T, nx, nu, dev) for k in libs}
    calls = {k: _hard_loop_call(lib, p, T, outs[k]) for k, lib in libs.items()}
    med = {k: [] for k in libs}
    for _ in range(a.rounds):
        for k in libs:
            med[k].append(_median_ms(calls[k], a.warmup, a.repeats)[0])
    for k in libs:
        res[f"hard_{k}_round_medians_ms"] = med[k]
        res[f"hard_{k}_ms"] = float(np.median(med[k]))
        res[f"hard_{k}_steps_per_s"] = b * T / (res[f"hard_{k}_ms"] * 1e-3)
    if a.ab_lib:
        res["hard_outputs_equal"] = all(
            np.array_equal(outs["this"][k].cpu().numpy(), outs["other"][k].cpu().numpy(),
                           equal_nan=k != "status") for k in ("xs", "us", "status"))
    res["hard"] = _stats(outs["this"])
    return outs["this"]


def affine_mode(a, dev):
    b, T = a.batch, a.steps
    rate = lambda ms: b * T / (ms * 1e-3)  # noqa: E731
    p = _config4(b, dev) if a.config4 else _session2(b, dev)
    qp, A, B, x0, hl, hu, E = (p[k] for k in ("qp", "A", "B", "x0", "hl", "hu", "E"))
    nx, nu, n = A.shape[0], B.shape[1], qp.n
    N = n // nu
    f64 = dict(dtype=torch.float64, device=dev)
    res = dict(tool="poly_loop_rate", mode="affine", problem=p["name"], batch=b, steps=T, n=n,
               m_total=qp.mt, repeats=a.repeats, rounds=a.rounds)
    _ab_hard(a, p, T, dev, res)                                            # (i)

    # the reference: a ramp on the first state that levels off, the rest at 0
    if a.config4:
        Q, R = torch.eye(nx, **f64), 0.1 * torch.eye(nu, **f64)
        ramp = np.minimum(0.05 * np.arange(T + N + 1), 1.0)
    else:
        pr = Problem()
        Q, R = (torch.as_tensor(np.asarray(v, float), **f64) for v in (pr.Q, pr.R))
        ramp = np.minimum(-40.0 + 6.0 * np.arange(T + N + 1), 0.0)
    cd = batched.condense(A, B, Q, R, Q, N, outputs=("H", "Gam"))
    x_ref = torch.zeros((T + N + 1, nx), **f64)
    x_ref[:, 0] = torch.as_tensor(ramp, **f64)
    g = batched.tracking_terms({"Gam": cd["Gam"][0]}, Q, R, Q, N, T, x_ref)   # (T, n)
    gb = g[:, None].expand(T, b, n).contiguous()

    def loop_run(gg):
        # a direct call like the hard loop's, so that both are timed alike
        o = _outs(b, T, nx, nu, dev)
        sb = qp.affine_scratch_bytes(b, T, gg.ndim == 2)
        scratch = torch.empty((sb,), dtype=torch.uint8, device=dev)
        ptr = batched._ptr
        lib = nat.load()
        args = (nat.F64, b, n, qp.m, qp.nbox, nx, nu, T, 0, ptr(qp.ws), ptr(E), ptr(A), ptr(B),
                ptr(x0), nx, ptr(hl), ptr(hu), 0, ptr(qp.lbz), ptr(qp.ubz), None, None, None,
                ptr(gg), 0 if gg.ndim == 2 else n, None, 0, ptr(scratch), sb, ptr(o["xs"]),
                ptr(o["us"]), None, None, None, ptr(o["status"]), 0, 0.0, batched._stream())

        def fn():
            rc = lib.mpcqp_mpc_poly_loop_affine(*args)
            assert rc == 0, rc
        ms = _median_ms(fn, a.warmup, a.repeats)[0]
        return o, dict(ms=ms, steps_per_s=rate(ms), ms_over_hard=ms / res["hard_this_ms"],
                       **_stats(o))

    o_sh, res["affine_shared_g"] = loop_run(g)                             # (ii)
    o_pi, res["affine_per_instance_g"] = loop_run(gb)                      # (iii)
    res["shared_equals_per_instance"] = all(
        np.array_equal(o_sh[k].cpu().numpy(), o_pi[k].cpu().numpy(), equal_nan=k != "status")
        for k in ("xs", "us", "status"))
    extra = res["affine_per_instance_g"]["ms"] - res["affine_shared_g"]["ms"]
    res["per_instance_prep_ms"] = extra
    res["per_instance_prep_share"] = extra / res["affine_per_instance_g"]["ms"]
    res["prep_macs_per_step"] = (n + qp.mt) * n

    # (iv) the per-step path with f = g_t, T steps in one HIP graph
    xs = torch.empty((T + 1, b, nx), **f64)
    zs = torch.empty((T, b, n), **f64)
    y = torch.empty((b, qp.mt), **f64)
    st = torch.empty((T, b), dtype=torch.int32, device=dev)
    hlt = None if hl is None or E is None else torch.empty((b, qp.m), **f64)
    hut = None if hu is None or E is None else torch.empty((b, qp.m), **f64)
    Et = None if E is None else E.T.contiguous()
    At, Bt = A.T.contiguous(), B.T.contiguous()
    tmp = torch.empty((b, nx), **f64)

    def episode():
        xs[0].copy_(x0)
        for t in range(T):
            x = xs[t]
            if Et is not None:
                torch.addmm(hl, x, Et, alpha=-1.0, out=hlt)
                torch.addmm(hu, x, Et, alpha=-1.0, out=hut)
                qp.solve(x, g[t], hlt, hut, out=(zs[t], y, st[t]))
            else:
                qp.solve(x, g[t], hl, hu, out=(zs[t], y, st[t]))
            torch.mm(x, At, out=tmp)
            torch.addmm(tmp, zs[t, :, :nu], Bt, out=xs[t + 1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        episode()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        episode()
    ms_step = _median_ms(graph.replay, a.warmup, a.repeats)[0]
    torch.cuda.synchronize()
    both = (((o_sh["status"] & 0xFF) == 0) & ((st & 0xFF) == 0)).all(dim=0)
    res["per_step_graph"] = dict(
        ms=ms_step, steps_per_s=rate(ms_step),
        optimal_fraction=((st & 0xFF) == 0).double().mean().item(),
        max_abs_x_diff_vs_loop=((o_sh["xs"][:, both] - xs[:, both]).abs().max().item()
                                if both.any() else float("nan")))
    res["speedup_shared_g_vs_per_step"] = ms_step / res["affine_shared_g"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config4", action="store_true")
    ap.add_argument("--soft", action="store_true")
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=None, help="--soft: N of the session-2 problem")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.repeats >= 10
    dev = torch.device("cuda:0")
    if a.soft or a.affine:
        line = json.dumps((affine_mode if a.affine else soft_mode)(a, dev))
        print(line)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "a") as f:
                f.write(line + "\n")
        return
    p = (_config4 if a.config4 else _session2)(a.batch, dev)
    qp, A, B, x0, hl, hu, E = (p[k] for k in ("qp", "A", "B", "x0", "hl", "hu", "E"))
    b, T, nx, nu, n = a.batch, a.steps, A.shape[0], B.shape[1], qp.n
    f64 = dict(dtype=torch.float64, device=dev)

    # ---- the one-launch loop, warm and cold
    outs = {}
    for cold in (False, True):
        o = dict(xs=torch.empty((T + 1, b, nx), **f64), us=torch.empty((T, b, nu), **f64),
                 status=torch.empty((T, b), dtype=torch.int32, device=dev))
        outs[cold] = (o, lambda o=o, cold=cold: qp.loop(A, B, x0, T, hl, hu, E, cold=cold, out=o))
    ms_warm = _median_ms(outs[False][1], a.warmup, a.repeats)
    ms_cold = _median_ms(outs[True][1], a.warmup, a.repeats)

    # ---- the per-step path, T steps in one HIP graph
    xs = torch.empty((T + 1, b, nx), **f64)
    zs = torch.empty((T, b, n), **f64)
    y = torch.empty((b, qp.mt), **f64)
    st = torch.empty((T, b), dtype=torch.int32, device=dev)
    hlt = None if hl is None or E is None else torch.empty((b, qp.m), **f64)
    hut = None if hu is None or E is None else torch.empty((b, qp.m), **f64)
    Et = None if E is None else E.T.contiguous()
    At, Bt = A.T.contiguous(), B.T.contiguous()
    tmp = torch.empty((b, nx), **f64)

    def episode():
        xs[0].copy_(x0)
        for t in range(T):
            x = xs[t]
            if Et is not None:
                torch.addmm(hl, x, Et, alpha=-1.0, out=hlt)
                torch.addmm(hu, x, Et, alpha=-1.0, out=hut)
                qp.solve(x, None, hlt, hut, out=(zs[t], y, st[t]))
            else:
                qp.solve(x, None, hl, hu, out=(zs[t], y, st[t]))
            torch.mm(x, At, out=tmp)
            torch.addmm(tmp, zs[t, :, :nu], Bt, out=xs[t + 1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        episode()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        episode()
    ms_step = _median_ms(graph.replay, a.warmup, a.repeats)
    torch.cuda.synchronize()

    ow, oc_ = outs[False][0], outs[True][0]
    code_w, code_s = ow["status"] & 0xFF, st & 0xFF
    both = ((code_w == 0) & (code_s == 0)).all(dim=0)       # instances optimal throughout in both
    diff = (ow["xs"][:, both] - xs[:, both]).abs().max().item() if both.any() else float("nan")
    it = lambda s: ((s[1:] >> 8) & 0xFFFF).double().mean().item()  # noqa: E731
    rate = lambda ms: b * T / (ms * 1e-3)  # noqa: E731
    res = dict(tool="poly_loop_rate", problem=p["name"], batch=b, steps=T, n=n, m_total=qp.mt,
               loop_warm_ms=ms_warm[0], loop_cold_ms=ms_cold[0], per_step_graph_ms=ms_step[0],
               loop_warm_steps_per_s=rate(ms_warm[0]), loop_cold_steps_per_s=rate(ms_cold[0]),
               per_step_graph_steps_per_s=rate(ms_step[0]),
               speedup_warm_vs_per_step=ms_step[0] / ms_warm[0],
               iters_warm_mean=it(ow["status"]), iters_cold_mean=it(oc_["status"]),
               iters_per_step_path_mean=it(st),
               optimal_fraction_loop=(code_w == 0).double().mean().item(),
               optimal_fraction_per_step=(code_s == 0).double().mean().item(),
               max_abs_x_diff_loop_vs_per_step=diff, repeats=a.repeats,
               min_ms=dict(warm=ms_warm[1], cold=ms_cold[1], per_step=ms_step[1]))
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
