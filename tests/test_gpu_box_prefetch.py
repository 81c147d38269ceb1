"""The Goldfarb-Idnani box active set of the four-QPs-per-wave layout
(gi_box_st, quad.hpp) where a change to how an iteration gets its pivot
column can go wrong (the cases were drawn up for a prefetch of that column,
DESIGN 3.3): partial steps (a bound is dropped, then the same pivot is tried
again), groups of one wave in different states, every block size with
padding, more than one pass of max_iter, the other two users of the active
set (mpcqp_solve_box and the warm-started mpcqp_mpc_box_loop), and the fused
kernel with and without a drift (which it neither stages nor reads when there
is none).

As in test_gpu_mpc_box_edges.py every fused call runs through both kernels
(mpc_group_kernel and the one-QP-per-wave comparator) and is held to the
oracle at 1e-9 * max(1, |z_ref|_inf) in fp64 and at _tol32 in fp32.
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import cbaseline
from oracle import condense as oc
from oracle import qp as oq
from test_gpu_loop_box import _check_episode, _episode
from test_gpu_mpc_box_edges import (PATHS, _check_vs_oracle, _fused, _n_active, _oracle, _refs,
                                    _tight_problem, _tol32)
from test_gpu_mpc_box_factor import _cfg2_plant, _t

pytestmark = pytest.mark.gpu

N2 = 20
# config-2 instances that drop a bound once and add it again (asserted below)
DROP_X0 = np.concatenate([np.array([8.0, -3.0]) * np.array([1.0, -1.0, 0.9, 1.1, -0.95, 1.2])[:, None],
                          np.array([[-8.18067443, 1.6134831], [7.56302712, -2.1333289]])])
LONG_X0 = np.array([-9.5, 6.5])      # needs >= 18 iterations (asserted below)


def _gi_model(H, f, lb, ub, tol=1e-9):
    """The kernels' dual active set in NumPy, for iteration counts only: from
    M = -H^-1 and z = M f, add the free row of largest relative violation; a
    ratio test over the active multipliers makes the step partial (the blocking
    bound is released, the same pivot is tried again) or full.  Returns
    (z, iterations)."""
    n = f.size
    M = -np.linalg.inv(H)
    st = np.zeros(n, int)
    mu = np.zeros(n)
    z = M @ f
    it = 0

    def sweep(k, sigma):
        d = M[k, k]
        col, row = M[:, k].copy(), M[k, :].copy()
        M[:] = M - np.outer(col, row) / d
        M[k, :] = sigma * row / d
        M[:, k] = sigma * col / d
        M[k, k] = -1.0 / d

    while True:
        with np.errstate(invalid="ignore"):
            v = np.fmax((lb - z) / (1 + np.abs(lb)), (z - ub) / (1 + np.abs(ub)))
        v = np.where((st == 0) & np.isfinite(v), v, -np.inf)
        p = int(np.argmax(v))
        if not v[p] > tol:
            return z, it
        side = 1 if z[p] < lb[p] else 2
        tgt = lb[p] if side == 1 else ub[p]
        zp, gp = z[p], 0.0
        while True:
            it += 1
            assert it < 200
            c, rm = M[:, p], 1.0 / M[p, p]
            sgn = 1.0 if tgt > zp else -1.0
            cs = c * rm
            dmu = np.where(st == 1, -cs, np.where(st == 2, cs, 0.0)) * sgn
            cand = (st != 0) & (dmu < 0)
            t = np.where(cand, -mu / np.where(cand, dmu, 1.0), np.inf)
            k = int(np.argmin(t))
            partial = t[k] < abs(tgt - zp)
            s = t[k] if partial else abs(tgt - zp)
            z = np.where(st == 0, z + sgn * s * cs, z)
            mu = mu + s * dmu
            gp -= sgn * s * rm
            zp += sgn * s
            if partial:
                sweep(k, 1.0)
                st[k], mu[k] = 0, 0.0
            else:
                sweep(p, -1.0)
                st[p], z[p], mu[p] = side, tgt, (gp if side == 1 else -gp)
                break


def _cfg2(x0, lb=-1.0, ub=1.0):
    A, B, Q, R, Qf = _cfg2_plant()
    b = x0.shape[0]
    return dict(A=np.broadcast_to(A, (b, 2, 2)), B=np.broadcast_to(B, (b, 2, 1)), Q=Q, R=R, Qf=Qf,
                N=N2, x0=x0, lb=lb, ub=ub, c=None, tv=False)


_drop_cache = {}


def _drop_refs():
    """Oracle solutions of the DROP_X0 family and the iteration counts of the C
    oracle's dual active set, computed once."""
    if not _drop_cache:
        p = _cfg2(DROP_X0)
        refs = _refs(p, DROP_X0.shape[0])
        A, B, Q, R, Qf = _cfg2_plant()
        _, it = cbaseline.mpc_box(A, B, Q, R, Qf, N2, DROP_X0, -1.0, 1.0)
        _drop_cache.update(p=p, refs=refs, iters=it,
                           nact=np.array([_n_active(r[0], r[3], r[4]) for r in refs]))
    return _drop_cache


# ------------------------------------------- partial steps, then the same pivot
def test_drop_then_same_pivot_config2(dev, monkeypatch):
    d = _drop_refs()
    print("iterations", d["iters"].tolist(), "active", d["nact"].tolist())
    assert (d["iters"] - d["nact"] >= 2).all(), (d["iters"], d["nact"])
    for b, r in enumerate(d["refs"]):        # the model below counts as the C oracle does
        assert _gi_model(r[1], r[2], r[3], r[4])[1] == d["iters"][b], b
    out = _fused(dev, monkeypatch, **d["p"])
    _check_vs_oracle(out, [r[0] for r in d["refs"]])
    assert out["group"][2].tolist() == out["wave"][2].tolist()


def test_drop_time_varying_nu2(dev, monkeypatch):
    """nu = 2, time-varying, n = 20: at least half of the instances take more
    iterations than they end up with active bounds, i.e. drop a bound on the
    way (TV_EXTRA: a seed chosen on the oracle for that)."""
    batch = 8
    p, _ = _tight_problem(4, 2, 10, True, batch, extra=TV_EXTRA)
    refs = _refs(p, batch)
    nact = [_n_active(r[0], r[3], r[4]) for r in refs]
    its = []
    for r in refs:
        zm, it = _gi_model(r[1], r[2], r[3], r[4])
        assert np.abs(zm - r[0]).max() < 1e-9 * max(1, np.abs(r[0]).max())
        its.append(it)
    print("iterations", its, "active", nact)
    assert sum(i > k for i, k in zip(its, nact)) * 2 >= batch, (its, nact)
    out = _fused(dev, monkeypatch, **p)
    _check_vs_oracle(out, [r[0] for r in refs])


TV_EXTRA = 62


# ----------------------------------------- one wave, groups in different states
@pytest.mark.parametrize("batch", [1, 2, 3, 5, 7])
def test_groups_in_different_states(dev, monkeypatch, batch):
    """In one launch: a QP that drops a bound, one that settles at 0
    iterations, one that needs >= 18, an empty box, then more of the same; the
    batch sizes leave 3, 2, 1, 3 and 1 groups of the last wave dead."""
    x0 = np.array([DROP_X0[0], [0.0, 0.0], LONG_X0, DROP_X0[2], DROP_X0[6], -LONG_X0,
                   [0.0, 0.0]])[:batch]
    expect = [0, 0, 0, 3, 0, 0, 0][:batch]
    lb, ub = -np.ones((batch, N2)), np.ones((batch, N2))
    if batch > 3:
        lb[3, 7] = 1.5
    p = _cfg2(x0, lb, ub)
    good = [b for b in range(batch) if expect[b] == 0]
    refs = [_oracle(p["A"], p["B"], p["Q"], p["R"], p["Qf"], N2, x0, lb, ub, None, False, b)
            if b in good else None for b in range(batch)]
    A, B, Q, R, Qf = _cfg2_plant()
    _, it = cbaseline.mpc_box(A, B, Q, R, Qf, N2, x0, -1.0, 1.0)
    assert it[0] - _n_active(refs[0][0], refs[0][3], refs[0][4]) >= 2
    if batch > 1:
        assert it[1] == 0
    if batch > 2:
        assert it[2] >= 18, it
    out = _fused(dev, monkeypatch, **p)
    for path in PATHS:
        z, code, iters = out[path]
        assert code.tolist() == expect, (path, code)
        for b in range(batch):
            assert (np.isfinite(z[b]).all() if b in good else np.isnan(z[b]).all()), (path, b)
        if batch > 1:
            assert iters[1] == 0, (path, iters)
    _check_vs_oracle(out, [r[0] if r is not None else None for r in refs], which=good)


# ------------------------------------------------- every block size and padding
# (nx, nu, N, tv): n = 1, 3, 4, 5, 17, 20, 21, 32 at nu = 1 and n = 18, 32 at
# nu = 2: block sizes 1, 1, 1, 2, 5, 5, 6, 8 and 5, 8, with rows past n inside a
# block at n = 1, 3, 5, 17, 21 and 18
BS_SHAPES = [(2, 1, 1, False), (2, 1, 3, True), (2, 1, 4, False), (2, 1, 5, True), (2, 1, 17, True),
             (2, 1, 20, False), (3, 1, 21, True), (4, 1, 32, False), (2, 2, 9, True),
             (4, 2, 16, True)]
BS_BATCH = 6
_bs_cache = {}


def _bs_problem(nx, nu, N, tv, fp32):
    """Tight bounds and the oracle on the (fp32: fp32-rounded) plant, once."""
    key = (nx, nu, N, tv, fp32)
    if key not in _bs_cache:
        p, _ = _tight_problem(nx, nu, N, tv, BS_BATCH, extra=BS_EXTRA)
        q = dict(p)
        if fp32:
            q["A"] = p["A"].astype(np.float32).astype(np.float64)
            q["B"] = p["B"].astype(np.float32).astype(np.float64)
        _bs_cache[key] = (p, _refs(q, BS_BATCH))
    return _bs_cache[key]


BS_EXTRA = 8


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("nx,nu,N,tv", BS_SHAPES)
def test_block_sizes(dev, monkeypatch, nx, nu, N, tv, fp32):
    p, refs = _bs_problem(nx, nu, N, tv, fp32)
    nact = [_n_active(r[0], r[3], r[4]) for r in refs]
    print("active bounds per instance", nact, "of", N * nu)
    assert sum(k > 0 for k in nact) > BS_BATCH // 2, nact
    if fp32:
        out = _fused(dev, monkeypatch, dt=torch.float32, **p)
        _check_vs_oracle(out, [r[0] for r in refs], tol=[_tol32(r[1]) for r in refs])
    else:
        out = _fused(dev, monkeypatch, **p)
        _check_vs_oracle(out, [r[0] for r in refs])


# ------------------------------------------------------- more than one `pass`
def test_max_iter_ladder(dev, monkeypatch):
    """max_iter from 1 to each instance's own iteration count on the DROP_X0
    family: MAXITER below the count and OPTIMAL (the oracle's z) at it, z always
    finite and inside the box, the reported count non-decreasing."""
    d = _drop_refs()
    full = _fused(dev, monkeypatch, **d["p"])
    for path in PATHS:
        assert (full[path][1] == 0).all()
    count = {path: full[path][2] for path in PATHS}
    top = int(max(c.max() for c in count.values()))
    assert top >= 8
    prev = {path: np.zeros(DROP_X0.shape[0], int) for path in PATHS}
    for m in range(1, top + 1):
        out = _fused(dev, monkeypatch, max_iter=m, **d["p"])
        for path in PATHS:
            z, code, iters = out[path]
            assert code.tolist() == [1 if m < c else 0 for c in count[path]], (path, m, code)
            assert np.isfinite(z).all() and (z >= -1.0).all() and (z <= 1.0).all(), (path, m)
            assert (iters >= prev[path]).all(), (path, m, iters, prev[path])
            prev[path] = iters
            for b, r in enumerate(d["refs"]):
                if code[b] == 0:
                    assert np.abs(z[b] - r[0]).max() < 1e-9 * max(1, np.abs(r[0]).max()), (path, m, b)


# ---------------------------------- the other users: solve_box and the box loop
def test_solve_box_on_drop_instances(dev):
    """mpcqp_solve_box (box_quad_kernel) on the packed H of batched.condense."""
    d = _drop_refs()
    p = d["p"]
    t = lambda a: _t(a, dev)  # noqa: E731
    cd = batched.condense(t(p["A"]), t(p["B"]), t(p["Q"]), t(p["R"]), t(p["Qf"]), N2, x0=t(p["x0"]),
                          outputs=("H", "f"))
    z, st = batched.solve_box(cd["H"], cd["f"], -1.0, 1.0)
    torch.cuda.synchronize()
    assert (batched.status_code(st) == 0).all()
    z = z.cpu().numpy()
    for b, r in enumerate(d["refs"]):
        err = np.abs(z[b] - r[0]).max()
        print(f"b={b}: err {err:.2e}")
        assert err < 1e-9 * max(1, np.abs(r[0]).max()), (b, err)


def test_box_loop_on_drop_instances(dev):
    """Five steps of mpcqp_mpc_box_loop (the warm-started active set) from the
    same states, step by step against the oracle at the device's own states."""
    A, B, Q, R, Qf = _cfg2_plant()
    t = lambda a: _t(a, dev)  # noqa: E731
    r = _episode(batched.mpc_box_loop(t(A), t(B), t(Q), t(R), t(Qf), N2, t(DROP_X0), -1.0, 1.0, 5,
                                      plans=True))
    assert ((r["status"] & 0xFF) == 0).all(), r["status"] & 0xFF
    cd = oc.condense(A, B, Q, R, Qf, N2)
    for i in range(DROP_X0.shape[0]):
        _check_episode(A, B, cd["H"], cd["F"], -1.0, 1.0, r["xs"], r["us"], r["zs"], i)


# ------------------------------------------------------- with and without drift
@pytest.mark.parametrize("nx,nu,N,tv", [(2, 1, 20, False), (2, 2, 9, True), (3, 1, 12, False),
                                        (4, 2, 8, True)])
def test_drift_none_zero_nonzero(dev, monkeypatch, nx, nu, N, tv):
    """c = None and c = 0 give bitwise equal z, status and iteration counts; a
    non-zero drift equals the oracle (LTI and time-varying, nx <= 2 and nx > 2:
    the two forms of the free-response loop)."""
    batch = 6
    p, rng = _tight_problem(nx, nu, N, tv, batch, extra=9)
    drift = rng.normal(size=(batch, N, nx)) * 0.3
    p["c"] = None
    none = _fused(dev, monkeypatch, **p)
    p["c"] = np.zeros((batch, N, nx))
    zero = _fused(dev, monkeypatch, **p)
    for path in PATHS:
        for k in range(3):
            assert np.array_equal(none[path][k], zero[path][k]), (path, k)
    refs = _refs(p, batch)
    assert sum(_n_active(r[0], r[3], r[4]) > 0 for r in refs) > batch // 2
    _check_vs_oracle(none, [r[0] for r in refs])
    p["c"] = drift
    refs = _refs(p, batch)
    assert sum(_n_active(r[0], r[3], r[4]) > 0 for r in refs) > batch // 2
    _check_vs_oracle(_fused(dev, monkeypatch, **p), [r[0] for r in refs])
