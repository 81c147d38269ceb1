"""The full-step path of the box active set at fp64 BS = 5 with a sweep of its own
(`MPCQP_FULL_SWEEP`, gi_box_trip.inc): a wave on the full-step path sweeps inside
the path, on the pivot's column still in registers with sigma = -1 folded in; a wave on the
general path sweeps behind the paths as before.  Both sweeps work on the one M of a lane, and
a wave changes from one to the other whenever the ratio filter of any of its four groups says
so.  What can go wrong is therefore the hand-over, and what the own sweep does for groups
that do not sweep (settled, stopped, not convex).  `MPCQP_PUBLISH_NODRAIN` moves a wait and
no value; the pivot cases below run every address of the column block all the same.

1. path changes inside a wave: one group takes its one partial step in trip t while its three
   neighbours take full steps, and all take full steps again in t + 1 (full -> general ->
   full), with t as early (trip 2: trip 1 of a cold start has no active bound that could
   block), in the middle, and as late (the trip before the last: a partial step is always
   followed by the full step of the same pivot) as the method allows; mpcqp_solve_box at
   n = 20 and 17 and the fused kernel at N = 20 and 17;
2. uneven finish: groups that settle after 0, 4 and 6 trips next to one that takes 20, and
   max_iter = 1, 2, 3 on that wave;
3. NOT_CONVEX met on the full-step path between optimal neighbours;
4. a pivot at every position (the cases of test_gpu_box_trip_lean.py) at batches 4, 5, 7, 64;
5. the fused kernel over the grid of x0 from no active bound to all, N = 20 and 17, against
   the oracle and the split pipeline, batches 4, 5, 7 bit-equal to the rows of the full one.

References and tolerances are those of test_gpu_box_fasttrip.py and
test_gpu_box_trip_lean.py: oracle/qp.box_qp for z (TOL), the restatement `_gi` for status
words and for the trip in which an instance takes its partial step, the split pipeline
(1e-9), and bit equality between the same instance in different waves.
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import qp as oq
from test_gpu_box_fasttrip import (DROP_X0, FULL_X0, MAXITER, NOT_CONVEX, OPTIMAL, TOL, _cfg2_qp,
                                   _gi, _pack, _plant2, _t, _word)
from test_gpu_box_trip_lean import GRID_X0, SIZES, _grid_refs, _pivot_cases, _solve

gpu = pytest.mark.gpu


def _bits(z):
    return np.ascontiguousarray(z).view(np.uint64)


def _partial_trips(H, f, lb, ub):
    """(status code, trips, the trips that were partial steps) by the restatement: the
    partial steps among the first m trips, for m = 1 .. trips."""
    _, code, it, parts = _gi(H, f, lb, ub)
    trips, prev = [], 0
    for m in range(1, it + 1 if parts else 1):
        q = _gi(H, f, lb, ub, max_iter=m)[3]
        if q > prev:
            trips.append(m)
        prev = q
    return code, it, trips


# --------------------------------------------------- 1. path changes inside a wave
def _rand_qp(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n, n))
    return G @ G.T + 0.3 * np.eye(n), 4 * rng.normal(size=n)


# seeds of _rand_qp by what the restatement says of them (asserted in _hand_over): X takes
# full steps only; the others take one partial step, in trip 2, in between, in the last but one
SEEDS = {20: dict(X=7, early=1780, mid=51, late=61), 17: dict(X=29, early=193, mid=20, late=175)}
KINDS = ["early", "mid", "late"]
_ho_cache = {}


def _hand_over(n):
    """{name: (H, f, z of the oracle, status word, trips, partial trips)}, once per n."""
    if n not in _ho_cache:
        lb, ub = -np.ones(n), np.ones(n)
        out = {}
        for name, seed in SEEDS[n].items():
            H, f = _rand_qp(n, seed)
            code, it, trips = _partial_trips(H, f, lb, ub)
            assert code == OPTIMAL, (n, name)
            out[name] = (H, f, oq.box_qp(H, f, lb, ub)[0], _word(code, it), it, trips)
        _ho_cache[n] = out
    return _ho_cache[n]


@pytest.mark.parametrize("n", SIZES)
def test_hand_over_cases_are_what_they_are_called(n):
    c = _hand_over(n)
    assert c["X"][5] == []
    for kind in KINDS:
        it, trips = c[kind][4], c[kind][5]
        assert len(trips) == 1, (n, kind, trips)
        t = trips[0]
        assert (t == 2) if kind == "early" else (t == it - 1) if kind == "late" else 2 < t < it - 1
        # the neighbours are still stepping in t and t + 1, and the group itself in t + 1
        assert c["X"][4] >= t + 1 and it >= t + 1, (n, kind, c["X"][4], it, t)


def _check(z, st, b, case, tag):
    err = np.abs(z[b] - case[2]).max()
    assert st[b] == case[3], (tag, b, st[b], case[3])
    assert err < TOL * max(1, np.abs(case[2]).max()), (tag, b, err)
    return err


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_full_general_full_solve_box(dev, n, kind):
    c = _hand_over(n)
    X, Y = c["X"], c[kind]
    z, st = _solve(dev, [X, Y, X, X])            # batch 4: one wave
    zx, stx = _solve(dev, [X, X, X, X])
    zy, sty = _solve(dev, [Y, Y, Y, Y])
    errs = [_check(z, st, b, case, (n, kind)) for b, case in enumerate([X, Y, X, X])]
    print(f"n={n} {kind}: Y {Y[4]} trips, partial in {Y[5]}, X {X[4]} trips, max err {max(errs):.2e}")
    for b in (0, 2, 3):                           # X does not see which path the wave took
        assert stx[b] == st[b] and np.array_equal(_bits(z[b]), _bits(zx[0])), (n, kind, b)
    assert (sty == st[1]).all() and all(np.array_equal(_bits(zy[b]), _bits(z[1])) for b in range(4))


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_full_general_full_batches(dev, n):
    """64 instances: the group that changes the wave's path at every position of a wave, the
    three kinds in turn; batches of 5 and 7 are the same rows, bit for bit."""
    c = _hand_over(n)
    cases = []
    for w in range(16):
        wave = [c["X"]] * 4
        wave[w % 4] = c[KINDS[(w // 4) % 3]]
        if w == 15:
            wave = [c[k] for k in ("early", "mid", "late", "X")]     # three changes in one wave
        cases += wave
    z, st = _solve(dev, cases)
    for b, case in enumerate(cases):
        _check(z, st, b, case, n)
    for batch in (5, 7):
        zb, stb = _solve(dev, cases[:batch])
        assert np.array_equal(stb, st[:batch]), (n, batch)
        assert np.array_equal(_bits(zb), _bits(z[:batch])), (n, batch)


def _mpc_box(dev, N, x0, **kw):
    A, B, Q, R, Qf = _plant2()
    t = lambda a: _t(a, dev)  # noqa: E731
    z, st = batched.mpc_box(t(A), t(B), t(Q), t(R), t(Qf), N, t(np.asarray(x0)), -1.0, 1.0, **kw)
    torch.cuda.synchronize()
    return z.cpu().numpy(), st.cpu().numpy()


@gpu
@pytest.mark.parametrize("d", [0, 2])
@pytest.mark.parametrize("N", SIZES)
def test_full_general_full_fused(dev, N, d):
    """The config-2 plant: F takes N full steps, D drops a bound in trip 6 (d = 0) or 7 (d = 2,
    the last but one) of 8; the family has no instance with an earlier partial step."""
    lb, ub = -np.ones(N), np.ones(N)
    F, D = FULL_X0[0], DROP_X0[d]
    code, it, trips = _partial_trips(*_cfg2_qp(D, N), lb, ub)
    assert (code, it, trips) == (OPTIMAL, 8, [6 if d == 0 else 7])
    assert _partial_trips(*_cfg2_qp(F, N), lb, ub) == (OPTIMAL, N, [])
    z, st = _mpc_box(dev, N, [F, D, F, F])
    zf, stf = _mpc_box(dev, N, [F, F, F, F])
    zd, std = _mpc_box(dev, N, [D, D, D, D])
    for b, x in enumerate([F, D, F, F]):
        H, f = _cfg2_qp(x, N)
        zr, code, it, _ = _gi(H, f, lb, ub)
        zo = oq.box_qp(H, f, lb, ub)[0]
        assert st[b] == _word(code, it), (N, d, b, st[b], code, it)
        assert np.abs(z[b] - zo).max() < TOL * max(1, np.abs(zo).max()), (N, d, b)
    for b in (0, 2, 3):
        assert stf[b] == st[b] and np.array_equal(_bits(z[b]), _bits(zf[0])), (N, d, b)
    assert (std == st[1]).all() and all(np.array_equal(_bits(zd[b]), _bits(z[1])) for b in range(4))


# ------------------------------------------------------------ 2. uneven finish
UNEVEN_X0 = np.array([FULL_X0[0], [0.0, 0.0], FULL_X0[3], FULL_X0[1]])   # 20, 0, 4, 6 trips


def test_uneven_wave_settles_at_different_trips():
    lb, ub = -np.ones(20), np.ones(20)
    its = [_gi(*_cfg2_qp(x), lb, ub)[1:] for x in UNEVEN_X0]
    assert its == [(OPTIMAL, 20, 0), (OPTIMAL, 0, 0), (OPTIMAL, 4, 0), (OPTIMAL, 6, 0)], its


@gpu
@pytest.mark.parametrize("kernel", ["solve_box", "fused"])
@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_uneven_finish(dev, kernel, m):
    """m = 0: no limit, the groups settle after 20, 0, 4 and 6 trips; m = 1, 2, 3: the limit
    stops three of them while the second has settled.  Status word and z of the restatement
    (after a stop: the bounds set so far, the rest from the exact refresh)."""
    lb, ub = -np.ones(20), np.ones(20)
    qps = [_cfg2_qp(x) for x in UNEVEN_X0]
    kw = dict(max_iter=m) if m else {}
    if kernel == "fused":
        z, st = _mpc_box(dev, 20, UNEVEN_X0, **kw)
    else:
        z, st = _solve(dev, qps, **kw)
    for b, (H, f) in enumerate(qps):
        zr, code, it, _ = _gi(H, f, lb, ub, max_iter=m)
        assert code == (MAXITER if m and b != 1 else OPTIMAL)
        assert st[b] == _word(code, it), (kernel, m, b, st[b], code, it)
        assert np.isfinite(z[b]).all() and (np.abs(z[b]) <= 1.0).all(), (kernel, m, b)
        assert np.abs(z[b] - zr).max() < TOL * max(1, np.abs(zr).max()), (kernel, m, b)


# -------------------------------------------------------------- 3. NOT_CONVEX
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_not_convex_on_the_full_step_path(dev, n):
    """M_pp >= 0 at the first pivot of one group, in a wave whose groups take full steps only:
    the path's own sweep must leave that group alone (`bad`: no sweep) and its neighbours'
    results are those of a wave without it, bit for bit."""
    X = _hand_over(n)["X"]
    Hbad = X[0].copy()
    p = int(np.argmax(np.abs(np.linalg.solve(X[0], X[1]))))
    Hbad[p, p] = -abs(X[0][p, p])
    for pos in range(4):
        wave = [X] * 4
        wave[pos] = (Hbad, X[1])
        z, st = _solve(dev, wave)
        zx, _ = _solve(dev, [X] * 4)
        assert (st[pos] & 0xFF) == NOT_CONVEX and np.isnan(z[pos]).all(), (n, pos, st)
        for b in range(4):
            if b != pos:
                assert st[b] == X[3], (n, pos, b, st)
                assert np.array_equal(_bits(z[b]), _bits(zx[b])), (n, pos, b)


# ------------------------------------------------- 4. a pivot at every position
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_pivot_position_at_every_batch(dev, n):
    base = _pivot_cases(n)                          # n singles + 16 pairs: (H, f, rows, z, word)
    cases = (base + base)[:64]
    z, st = _solve(dev, cases)
    for b, (_, _, ks, zo, word) in enumerate(cases):
        assert st[b] == word, (n, ks, st[b], word)
        assert np.abs(z[b] - zo).max() < TOL * max(1, np.abs(zo).max()), (n, ks)
    assert np.array_equal(_bits(z[len(base):]), _bits(z[:64 - len(base)]))
    for batch in (4, 5, 7):
        zb, stb = _solve(dev, cases[:batch])
        assert np.array_equal(stb, st[:batch]), (n, batch)
        assert np.array_equal(_bits(zb), _bits(z[:batch])), (n, batch)


# ------------------------------------------------------ 5. the fused kernel's grid
@gpu
@pytest.mark.parametrize("N", SIZES)
def test_fused_grid_and_batch_tails(dev, N):
    A, B, Q, R, Qf = _plant2()
    t = lambda a: _t(a, dev)  # noqa: E731
    x0 = np.concatenate([GRID_X0] * 5)[:64]
    z, st = _mpc_box(dev, N, x0)
    d = batched.condense(t(A), t(B), t(Q), t(R), t(Qf), N, x0=t(x0))
    zs, sts = batched.solve_box(d["H"], d["f"], -1.0, 1.0)
    torch.cuda.synchronize()
    assert ((st & 0xFF) == OPTIMAL).all() and (batched.status_code(sts) == 0).all()
    split = np.abs(z - zs.cpu().numpy()).max()
    zo, nact = _grid_refs(N)
    assert nact.min() == 0 and nact.max() == N
    for b in range(64):
        r = zo[b % len(GRID_X0)]
        assert np.abs(z[b] - r).max() < TOL * max(1, np.abs(r).max()), (N, b)
    print(f"N={N}: fused vs split {split:.2e}")
    assert split < 1e-9, split
    for batch in (4, 5, 7):
        zb, stb = _mpc_box(dev, N, x0[:batch])
        assert np.array_equal(stb, st[:batch]), (N, batch)
        assert np.array_equal(_bits(zb), _bits(z[:batch])), (N, batch)
