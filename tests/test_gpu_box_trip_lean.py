"""The leaner trip of the box active set at fp64 BS = 5 (gi_box_core.hpp, quad.hpp; DESIGN
3.3): the sweep writes row k and column k of the pivot as 64-bit moves under lane masks
(`QSym::sweep_col<RD, true>`), and the multiplier rates are formed once per trip for the
filter, the ratio test and the step.  Neither changes an operand or an operation, so what
is checked here is where the masked moves can go wrong and what the shared rates feed:

1. a pivot at every position: for each k one QP whose optimum has exactly bound k active,
   and pairs (k, l) over all 4 x 4 combinations of the two pivots' blocks with every
   in-block offset, at n = 20 and n = 17 (BS = 5, the second with padding rows), batched so
   that the four groups of a wave pivot on different blocks and offsets in the same trip,
   and again as batches of 5 and 7 (idle groups in the last wave);
2. both paths in one wave: groups that drop a bound next to groups that take full steps
   only, and a batch that never leaves the full-step trip;
3. the fused kernel and the loop kernel (which shares the trip but keeps the select form
   and the per-use rates, `LoopLean`) on the config-2 plant over a grid of x0 from
   unsaturated to fully saturated, against the oracle and against the split pipeline;
4. status edges: max_iter 1, 2, 3 on an instance that needs 20 trips, and NOT_CONVEX
   between optimal neighbours whose results must not depend on it.

Only QSym<double, 5> takes the two pieces, so there is no case for another block size or
precision.  References: oracle/qp.box_qp for z; the restatement `_gi` of
test_gpu_box_fasttrip.py (the method in NumPy, on the CPU) for status words and for which
instance drops a bound.  Tolerances are those of test_gpu_box_fasttrip.py.
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import condense as oc
from oracle import qp as oq
from test_gpu_box_fasttrip import (DROP_X0, FULL_X0, MAXITER, NOT_CONVEX, OPTIMAL, TOL, _cfg2_qp,
                                   _gi, _pack, _plant2, _t, _word)
from test_gpu_loop_box import _check_episode, _episode

gpu = pytest.mark.gpu
BS = 5
SIZES = [20, 17]


# ------------------------------------------------------------ 1. pivot positions
def _pivot_qp(n, ks, seed):
    """H = I + G G' / (4 n) (weak coupling) and f = -H z0 with |z0| <= 0.3 but on the rows
    ks, which sit at +/- 1.6: on the box [-1, 1] exactly those bounds are active at the
    optimum (asserted on the oracle in _pivot_cases)."""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n, n))
    H = np.eye(n) + 0.25 * G @ G.T / n
    z0 = rng.uniform(-0.3, 0.3, n)
    for j, k in enumerate(ks):
        z0[k] = 1.6 if (k + j) % 2 == 0 else -1.6
    return H, -H @ z0


def _pivot_rows(n):
    """The single pivots, ordered so that four consecutive ones (a wave) lie in different
    blocks at different offsets, then the pairs: block a x block b with offsets that run
    through 0 .. 4 (0 .. n - 16 in a last block with padding)."""
    singles = [[k] for j in range(BS) for a in range(4) for k in [BS * a + (j + a) % BS] if k < n]
    pairs = []
    for a in range(4):
        for b in range(4):
            wa, wb = min(BS, n - BS * a), min(BS, n - BS * b)
            k, l = BS * a + (a + 2 * b) % wa, BS * b + (3 * a + b + 1) % wb
            if k == l:
                l = BS * b + (l - BS * b + 1) % wb
            pairs.append([k, l])
    return singles, pairs


_pivot_cache = {}


def _pivot_cases(n):
    """(H, f, rows, z of the oracle, status word of the restatement) per instance, once."""
    if n not in _pivot_cache:
        singles, pairs = _pivot_rows(n)
        lb, ub = -np.ones(n), np.ones(n)
        out = []
        for i, ks in enumerate(singles + pairs):
            H, f = _pivot_qp(n, ks, 100 * n + i)
            zo = oq.box_qp(H, f, lb, ub)[0]
            assert set(np.nonzero(np.abs(zo) >= 1 - 1e-12)[0]) == set(ks), (n, ks)
            _, code, it, parts = _gi(H, f, lb, ub)
            assert (code, it, parts) == (OPTIMAL, len(ks), 0), (n, ks, code, it, parts)
            out.append((H, f, ks, zo, _word(code, it)))
        _pivot_cache[n] = out
    return _pivot_cache[n]


@pytest.mark.parametrize("n", SIZES)
def test_pivot_cases_cover_every_position(n):
    singles, pairs = _pivot_rows(n)
    assert sorted(k for (k,) in singles) == list(range(n))
    for w in range(0, len(singles) - 3, 4):              # a wave: four blocks, four offsets
        ks = [k for (k,) in singles[w:w + 4]]
        if n == 20:
            assert len({k // BS for k in ks}) == 4 and len({k % BS for k in ks}) == 4, ks
    assert {(k // BS, l // BS) for k, l in pairs} == {(a, b) for a in range(4) for b in range(4)}
    assert all(k != l for k, l in pairs)
    for pos in (0, 1):
        assert {p[pos] % BS for p in pairs if p[pos] // BS < 3} == set(range(BS)), pairs
    assert len(_pivot_cases(n)) == n + 16


def _solve(dev, cases, **kw):
    Hs = np.stack([c[0] for c in cases])
    fs = np.stack([c[1] for c in cases])
    z, st = batched.solve_box(_t(_pack(Hs), dev), _t(fs, dev), -1.0, 1.0, **kw)
    torch.cuda.synchronize()
    return z.cpu().numpy(), st.cpu().numpy()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_pivot_position(dev, n):
    cases = _pivot_cases(n)
    z, st = _solve(dev, cases)
    for b, (_, _, ks, zo, word) in enumerate(cases):
        err = np.abs(z[b] - zo).max()
        assert st[b] == word, (n, ks, st[b], word)
        assert err < TOL * max(1, np.abs(zo).max()), (n, ks, err)
    print(f"n={n}: {len(cases)} instances, max err {max(np.abs(z[b] - c[3]).max() for b, c in enumerate(cases)):.2e}")
    # idle groups in the last wave: the same instances, the same bits
    for batch in (5, 7):
        zb, stb = _solve(dev, cases[:batch])
        assert np.array_equal(stb, st[:batch]), (n, batch)
        assert np.array_equal(zb.view(np.uint64), z[:batch].view(np.uint64)), (n, batch)


# ------------------------------------------------------ 2. both paths in one wave
def _cfg2_cases(x0s, n=20):
    lb, ub = -np.ones(n), np.ones(n)
    out = []
    for x0 in x0s:
        H, f = _cfg2_qp(x0, n)
        _, code, it, parts = _gi(H, f, lb, ub)
        out.append((H, f, parts, oq.box_qp(H, f, lb, ub)[0], _word(code, it)))
    return out


MIXED_X0 = [x for pair in zip(FULL_X0, DROP_X0[:4]) for x in pair]    # F D F D | F D F D
FULL_ONLY_X0 = list(FULL_X0) + list(FULL_X0[::-1])


def test_mixed_batch_has_both_kinds():
    parts = [c[2] for c in _cfg2_cases(MIXED_X0)]
    assert all(p >= 1 for p in parts[1::2]) and all(p == 0 for p in parts[0::2]), parts
    assert all(c[2] == 0 for c in _cfg2_cases(FULL_ONLY_X0))


@gpu
@pytest.mark.parametrize("kind", ["mixed", "full_only"])
def test_both_paths_in_one_wave(dev, kind):
    cases = _cfg2_cases(MIXED_X0 if kind == "mixed" else FULL_ONLY_X0)
    z, st = _solve(dev, cases)
    for b, (_, _, parts, zo, word) in enumerate(cases):
        err = np.abs(z[b] - zo).max()
        print(f"{kind} b={b}: partial steps {parts} iterations {st[b] >> 8} err {err:.2e}")
        assert st[b] == word, (kind, b, st[b], word)
        assert err < TOL * max(1, np.abs(zo).max()), (kind, b, err)


# ------------------------------------------------- 3. fused and loop kernels
GRID_X0 = np.array([[a, b] for a in (-9.5, -3.0, 0.2, 4.0, 10.0) for b in (-6.0, 0.1, 6.5)])
_grid_cache = {}


def _grid_refs(N):
    """Oracle z per grid point at horizon N and the number of active bounds."""
    if N not in _grid_cache:
        lb, ub = -np.ones(N), np.ones(N)
        zs = np.stack([oq.box_qp(*_cfg2_qp(x0, N), lb, ub)[0] for x0 in GRID_X0])
        _grid_cache[N] = (zs, (np.abs(zs) >= 1 - 1e-12).sum(axis=1))
    return _grid_cache[N]


@pytest.mark.parametrize("N", SIZES)
def test_grid_runs_from_unsaturated_to_saturated(N):
    nact = _grid_refs(N)[1]
    assert nact.min() == 0 and nact.max() == N and ((nact > 0) & (nact < N)).any(), nact


@gpu
@pytest.mark.parametrize("N", SIZES)
def test_fused_kernel_on_the_grid(dev, N):
    A, B, Q, R, Qf = _plant2()
    t = lambda a: _t(a, dev)  # noqa: E731
    z, st = batched.mpc_box(t(A), t(B), t(Q), t(R), t(Qf), N, t(GRID_X0), -1.0, 1.0)
    d = batched.condense(t(A), t(B), t(Q), t(R), t(Qf), N, x0=t(GRID_X0))
    zs, sts = batched.solve_box(d["H"], d["f"], -1.0, 1.0)
    torch.cuda.synchronize()
    assert (batched.status_code(st) == 0).all() and (batched.status_code(sts) == 0).all()
    split = float((z - zs).abs().max())
    z = z.cpu().numpy()
    zo, nact = _grid_refs(N)
    for b in range(len(GRID_X0)):
        err = np.abs(z[b] - zo[b]).max()
        assert err < TOL * max(1, np.abs(zo[b]).max()), (N, b, err)
    print(f"N={N}: active {nact.tolist()} fused vs split {split:.2e}")
    assert split < 1e-9, split                     # test_gpu_box.py: fused == split pipeline


@gpu
def test_loop_kernel_on_the_grid(dev):
    N, T = 20, 3
    A, B, Q, R, Qf = _plant2()
    t = lambda a: _t(a, dev)  # noqa: E731
    r = _episode(batched.mpc_box_loop(t(A), t(B), t(Q), t(R), t(Qf), N, t(GRID_X0), -1.0, 1.0, T,
                                      plans=True))
    assert ((r["status"] & 0xFF) == OPTIMAL).all(), r["status"]
    ref = oc.condense(A, B, Q, R, Qf, N, x0=np.zeros(2))
    for i in range(len(GRID_X0)):
        _check_episode(A, B, ref["H"], ref["F"], -1.0, 1.0, r["xs"], r["us"], r["zs"], i)


# ------------------------------------------------------------ 4. status edges
@gpu
def test_max_iter_ladder_on_twenty_bounds(dev):
    x0 = FULL_X0[0]
    lb, ub = -np.ones(20), np.ones(20)
    H, f = _cfg2_qp(x0)
    assert _gi(H, f, lb, ub)[2] == 20
    cases = [(H, f)] * 4
    for m in (1, 2, 3):
        zr, code, it, _ = _gi(H, f, lb, ub, max_iter=m)
        assert code == MAXITER
        z, st = _solve(dev, cases, max_iter=m)
        assert (st == _word(MAXITER, it)).all(), (m, st, it)
        assert np.isfinite(z).all() and (np.abs(z) <= 1.0).all(), m
        # the state the early exit leaves: m - 1 bounds set, the rest from the exact refresh
        assert np.abs(z - zr).max() < TOL * max(1, np.abs(zr).max()), (m, np.abs(z - zr).max())


@gpu
def test_not_convex_between_optimal_neighbours(dev):
    cases = _cfg2_cases([FULL_X0[1], DROP_X0[0], FULL_X0[2]])
    HX, fX = cases[0][0], cases[0][1]
    Hbad = HX.copy()
    p = int(np.argmax(np.abs(np.linalg.solve(HX, fX))))
    Hbad[p, p] = -abs(HX[p, p])
    z, st = _solve(dev, [cases[0], (Hbad, fX), cases[1], cases[2]])
    zr, str_ = _solve(dev, cases)
    assert (st[1] & 0xFF) == NOT_CONVEX, st
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert st[i] == str_[j] == cases[j][4], (i, st, str_)
        assert np.array_equal(z[i].view(np.uint64), zr[j].view(np.uint64)), i
