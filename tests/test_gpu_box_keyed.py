"""Keyed reductions in the box active set of the four-QPs-per-wavefront
kernels (quad.hpp, Key / RowOwn::keymax / keymin): in fp64 the scan, the ratio
test and the warm-start release scan reduce one key per lane -- the value with
its low KB = ceil(log2 NMAX) mantissa bits replaced by a code of the row index
-- instead of a (value, index, payload) triple, and z of a new pivot is read
from the owners' copy in LDS.

The cases go through mpcqp_solve_box (box_quad_kernel), through a short
mpcqp_mpc_box_loop (box_loop_kernel: step 0 cold, the others warm-started)
and, where a plant can produce them, through mpcqp_mpc_box (mpc_group_kernel).
The loop takes any H and any sequence of linear terms: it is handed
`condensed` = (H, F) with F = [f_0 .. f_{T-1}] and a plant that shifts a
one-hot state (B = 0), so that F x_t = f_t exactly.

References: the oracle (oracle/qp.py, KKT-certified) at 1e-9 * max(1, |z|_inf),
the tolerance of tests/test_gpu_box.py; the NumPy restatement of the method in
test_gpu_box_rowowner.py (`_gi_iterations`) for iteration counts; and the
one-QP-per-wavefront kernels (MPCQP_KERNEL=wave), which keep the
compare-and-select reductions.
"""
import numpy as np
import pytest
import torch

from model_predictive_control_amd import batched
from oracle import condense as oc
from test_gpu_box_rowowner import (PATHS, TOL, _check, _gi_iterations, _n_active, _oracle_box,
                                   _pack, _random_problems, _solve_box, _t)
from test_gpu_mpc_box_factor import _cfg2_plant

gpu = pytest.mark.gpu


# ------------------------------------------------------------- the key order
def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _key_pack(v, code, kb):
    mask = np.uint64((1 << kb) - 1)
    return ((_bits(v) & ~mask) | np.asarray(code, dtype=np.uint64)).view(np.float64)


def _key_clear(v, kb):
    return (_bits(v) & ~np.uint64((1 << kb) - 1)).view(np.float64)


def _key_big(kb):
    return _key_clear(np.array([np.finfo(np.float64).max]), kb)[0]


@pytest.mark.parametrize("kb", [2, 3, 4, 5])
def test_key_order_numpy(kb):
    """The packed comparison is (value, then the smaller index) whenever the
    values differ above the low kb bits or are exactly equal, for all index
    pairs; the sentinels order below / above every candidate and stay finite."""
    rng = np.random.default_rng(100 + kb)
    nmax, mask = 1 << kb, (1 << kb) - 1
    v = np.concatenate([rng.lognormal(0, 8, 40), [1.0, 1.0, 2.0 ** -1060, 1e300, 3.5, 3.5]])
    v = np.concatenate([v, np.nextafter(v[:8], np.inf), _key_clear(v[:8], kb)])
    a, b = np.meshgrid(v, v, indexing="ij")
    ca, cb = _key_clear(a, kb), _key_clear(b, kb)
    ok = (ca != cb) | (a == b)   # differ above the low bits, or exactly equal
    assert ok.sum() > v.size and (~ok).sum() > 0
    big = _key_big(kb)
    assert np.isfinite(big) and np.isfinite(_key_pack(big, mask, kb)).all()
    for i in range(nmax):
        for j in range(nmax):
            if i == j:
                continue
            want_a = (ca > cb) | ((ca == cb) & (i < j))          # a wins the arg-max
            got = _key_pack(a, mask - i, kb) > _key_pack(b, mask - j, kb)
            assert np.array_equal(got[ok], want_a[ok]), ("max", i, j)
            want_a = (ca < cb) | ((ca == cb) & (i < j))          # a wins the arg-min
            got = _key_pack(a, i, kb) < _key_pack(b, j, kb)
            assert np.array_equal(got[ok], want_a[ok]), ("min", i, j)
            want_a = (-ca < -cb) | ((ca == cb) & (i < j))        # arg-min of negative values
            got = _key_pack(-a, mask - i, kb) < _key_pack(-b, mask - j, kb)
            assert np.array_equal(got[ok], want_a[ok]), ("min-", i, j)
    # the winner unpacks to its index and to the value with its low bits clear
    k = _key_pack(v, mask - 3, kb)
    assert np.array_equal(mask - (_bits(k) & np.uint64(mask)).astype(int), np.full(v.size, 3))
    assert np.array_equal(_key_clear(k, kb), _key_clear(v, kb))
    # sentinels, with any code, against every candidate (clamped to +/- big)
    cand = np.concatenate([v, -v, [0.0, -0.0, big, -big]])
    cand = np.clip(cand, -big, big)
    for c in range(nmax):
        for c2 in (0, mask):
            assert (_key_pack(-big, c, kb) < _key_pack(cand[cand > -big], c2, kb)).all()
            assert (_key_pack(big, c, kb) > _key_pack(cand[cand < big], c2, kb)).all()


# ------------------------------------------------------------------ helpers
def _loop(dev, H, fseq, lb, ub, max_iter=0):
    """mpcqp_mpc_box_loop on QPs given as (H (b, n, n), f_t = fseq[t] (T, b, n)):
    z (T, b, n), codes and counts (sweeps + releases + iterations) (T, b)."""
    fseq = np.asarray(fseq, dtype=np.float64)
    T, b, n = fseq.shape
    nx = max(T, 2)
    A = np.zeros((nx, nx))
    A[np.arange(1, nx), np.arange(nx - 1)] = 1.0
    x0 = np.zeros((b, nx))
    x0[:, 0] = 1.0
    F = np.zeros((b, n, nx))
    F[:, :, :T] = fseq.transpose(1, 2, 0)
    cd = {"H": _t(_pack(H), dev), "F": _t(F, dev)}
    r = batched.mpc_box_loop(_t(A, dev), _t(np.zeros((nx, 1)), dev), None, None, None, n,
                             _t(x0, dev), _t(lb, dev), _t(ub, dev), T, plans=True,
                             max_iter=max_iter, condensed=cd)
    torch.cuda.synchronize()
    st = r["status"].cpu().numpy()
    return r["zs"].cpu().numpy(), st & 0xFF, (st >> 8) & 0xFFFF


def _shifted(prev, lb, ub):
    st0 = np.where(prev == lb, 1, np.where(prev == ub, 2, 0))
    return np.append(st0[1:], st0[-1])   # nu = 1


def _check_loop(dev, H, f, lb, ub, refs, counts=True):
    """Three steps with the same linear term: step 0 cold, steps 1 and 2 from
    the shifted active set of the step before.  Every step must give the
    oracle's z; with `counts`, as many sweeps + releases + iterations as the
    restatement started from the same states."""
    b, n = f.shape
    zs, code, its = _loop(dev, H, np.stack([f, f, f]), lb, ub)
    assert (code == 0).all(), code
    for t in range(3):
        for i in range(b):
            err = np.abs(zs[t, i] - refs[i]).max()
            assert err < TOL * max(1, np.abs(refs[i]).max()), (t, i, err)
            if counts:
                warm = np.zeros(n, int) if t == 0 else _shifted(zs[t - 1, i], lb[i], ub[i])
                want = _gi_iterations(H[i], f[i], lb[i], ub[i], warm=warm)[1]
                assert its[t, i] == want, (t, i, its[t, i], want)


def _twins(rng, m, batch, scale=8.0):
    """Two decoupled copies of one m-row QP: H = diag(A, A), f = (g, g), equal
    bounds.  Rows i and i + m carry the same numbers through the same
    arithmetic (the other half only ever adds exact zeros), so their
    violations are bit-equal at every scan."""
    Hs, fs, lbs, ubs = [], [], [], []
    for _ in range(batch):
        U, _ = np.linalg.qr(rng.normal(size=(m, m)))
        A = (U * np.logspace(0, 1.5, m)) @ U.T
        A = 0.5 * (A + A.T)
        H = np.zeros((2 * m, 2 * m))
        H[:m, :m] = H[m:, m:] = A
        g = rng.normal(size=m) * scale
        l, u = -rng.uniform(0.2, 2, m), rng.uniform(0.2, 2, m)
        Hs.append(H); fs.append(np.tile(g, 2)); lbs.append(np.tile(l, 2)); ubs.append(np.tile(u, 2))
    return np.array(Hs), np.array(fs), np.array(lbs), np.array(ubs)


# ------------------------------------------------------------------- ties
@gpu
@pytest.mark.parametrize("n", [8, 20])
def test_exact_ties(dev, monkeypatch, n):
    """Twin rows i and i + n/2 (n/2 = 2 BS: the same owner lane, two row blocks
    apart) tie bit for bit in every scan: the smaller index must pivot first.
    Status and iteration count equal the restatement's (np.argmax takes the
    first maximum) and the comparator's.  Cut after one iteration, only the
    first half has a row on a bound: the free rows of the first half have
    moved, those of the second half are still the unconstrained minimiser."""
    m, batch = n // 2, 5
    H, f, lb, ub = _twins(np.random.default_rng(8000 + n), m, batch)
    refs = [_oracle_box(H[b], f[b], lb[b], ub[b]) for b in range(batch)]
    want = [_gi_iterations(H[b], f[b], lb[b], ub[b])[1] for b in range(batch)]
    assert min(want) >= 2
    out = _solve_box(dev, monkeypatch, H, f, lb, ub)
    _check(out, refs)
    for path in PATHS:
        assert out[path][2].tolist() == want, (path, out[path][2], want)
    _check_loop(dev, H, f, lb, ub, refs)
    cut = _solve_box(dev, monkeypatch, H, f, lb, ub, max_iter=1)
    zl, codel, _ = _loop(dev, H, f[None], lb, ub, max_iter=1)
    for b in range(batch):
        zu = np.clip(-np.linalg.solve(H[b], f[b]), lb[b], ub[b])
        for name, z, code in [(p, cut[p][0][b], cut[p][1][b]) for p in PATHS] + [("loop", zl[0, b], codel[0, b])]:
            assert code == 1, (name, b, code)
            assert np.abs(z[m:] - zu[m:]).max() < TOL * max(1, np.abs(zu).max()), (name, b)
            assert np.abs(z[:m] - zu[:m]).max() > 1e-3, (name, b)
        assert np.abs(cut["group"][0][b] - cut["wave"][0][b]).max() < TOL * max(1, np.abs(zu).max())


@gpu
@pytest.mark.parametrize("n", [8, 20])
def test_near_ties(dev, monkeypatch, n):
    """The twins with the second copy's linear term moved by 1 .. 24 ulps:
    violations (and step lengths) that differ only in the last few mantissa
    bits, below what a key keeps.  Whichever row pivots first, the solution is
    the oracle's."""
    m, batch = n // 2, 6
    rng = np.random.default_rng(8100 + n)
    H, f, lb, ub = _twins(rng, m, batch)
    for b in range(batch):
        for i in range(m):
            for _ in range(int(rng.integers(1, 25))):
                f[b, m + i] = np.nextafter(f[b, m + i], np.inf if (b + i) % 2 else -np.inf)
    assert (f[:, :m] != f[:, m:]).all() and np.abs(f[:, :m] / f[:, m:] - 1).max() < 1e-14
    refs = [_oracle_box(H[b], f[b], lb[b], ub[b]) for b in range(batch)]
    _check(_solve_box(dev, monkeypatch, H, f, lb, ub), refs)
    _check_loop(dev, H, f, lb, ub, refs, counts=False)


# --------------------------------------------------------- infinite bounds
@gpu
def test_infinite_bounds_in_one_wave(dev, monkeypatch):
    """One wave holding an ordinary QP, one with one-sided bounds, one with
    rows unbounded on both sides and one without any finite bound; a second
    wave with one live group.  No NaN, every status optimal, the oracle's z;
    a row without a finite bound is never active: it ends at the value the
    stationarity of the free rows gives it."""
    n, batch = 20, 5
    rng = np.random.default_rng(8200)
    H, f, lb, ub = _random_problems(rng, n, batch)
    lb[0], ub[0] = -rng.uniform(0.1, 2, n), rng.uniform(0.1, 2, n)        # ordinary
    lb[1] = -np.inf                                                        # one side
    ub[1] = rng.uniform(0.1, 1, n)
    lb[3], ub[3] = -np.inf, np.inf                                         # every row
    refs = [_oracle_box(H[b], f[b], lb[b], ub[b]) for b in range(batch)]
    assert _n_active(refs[3], lb[3], ub[3]) == 0 and _n_active(refs[1], lb[1], ub[1]) > 2
    out = _solve_box(dev, monkeypatch, H, f, lb, ub)
    _check(out, refs)
    zs, code, _ = _loop(dev, H, np.stack([f, f, f]), lb, ub)
    assert (code == 0).all() and np.isfinite(zs).all()
    # (no counts: the restatement's arg-max does not skip the NaN violation of
    # a row without a finite bound)
    _check_loop(dev, H, f, lb, ub, refs, counts=False)
    for z in (out["group"][0], zs[0], zs[2]):
        assert np.isfinite(z).all()
        for b in range(batch):
            unb = np.isinf(lb[b]) & np.isinf(ub[b])
            grad = np.where(unb, H[b] @ z[b] + f[b], 0.0)
            assert np.abs(grad).max() < 1e-7 * max(1, np.abs(f[b]).max()), b


@gpu
def test_infinite_bounds_fused_step(dev):
    """mpcqp_mpc_box on the config-2 plant, N = 20, five instances in two
    waves: all bounds finite, lower bounds missing, rows unbounded on both
    sides, no finite bound at all, and an ordinary one."""
    A, B, Q, R, Qf = _cfg2_plant()
    N = 20
    x0 = np.array([[8.0, -3.0], [-9.5, 6.5], [7.6, -2.1], [-8.0, 3.0], [2.0, 1.5]])
    batch = x0.shape[0]
    lb, ub = -np.ones((batch, N)), np.ones((batch, N))
    lb[1] = -np.inf
    lb[2, ::3] = -np.inf
    ub[2, ::3] = np.inf
    lb[3], ub[3] = -np.inf, np.inf
    refs = []
    for b in range(batch):
        d = oc.condense(A, B, Q, R, Qf, N, x0=x0[b])
        refs.append(_oracle_box(d["H"], d["f"], lb[b], ub[b]))
    assert _n_active(refs[3], lb[3], ub[3]) == 0 and _n_active(refs[2], lb[2], ub[2]) > 0
    t = lambda a: _t(a, dev)  # noqa: E731
    z, st = batched.mpc_box(t(np.broadcast_to(A, (batch, 2, 2))), t(np.broadcast_to(B, (batch, 2, 1))),
                            t(Q), t(R), t(Qf), N, t(x0), t(lb), t(ub))
    torch.cuda.synchronize()
    z, code = z.cpu().numpy(), batched.status_code(st).cpu().numpy()
    assert np.isfinite(z).all()
    _check({"group": (z, code, None)}, refs, paths=("group",))


# -------------------------------------------- the ratio test's two outcomes
@gpu
def test_no_candidate_and_partial_then_same_pivot(dev, monkeypatch):
    """QP 0: one violated row and nothing active -- the ratio test has no
    candidate and the first step is a full one (1 iteration).  QPs 1..4: the
    restatement takes partial steps (a bound is dropped and the next
    iteration goes on with the same pivot).  Counts equal the restatement's."""
    n = 20
    rng = np.random.default_rng(8300)
    H, f, lb, ub = _random_problems(rng, n, 5)
    lb[np.isinf(lb)] = -1.5
    ub[np.isinf(ub)] = 1.5
    H[0] = np.eye(n) + 0.001 * H[0]
    f[0] = 0.0
    f[0, 7] = -9.0
    picked, seed = [], 0
    while len(picked) < 4:                      # deterministic: fixed seeds in order
        Hc, fc, lc, uc = _random_problems(np.random.default_rng(8310 + seed), n, 1)
        lc[np.isinf(lc)] = -1.5
        uc[np.isinf(uc)] = 1.5
        seed += 1
        if _gi_iterations(Hc[0], fc[0], lc[0], uc[0])[0] > 0:
            picked.append((Hc[0], fc[0], lc[0], uc[0]))
    for b, (Hc, fc, lc, uc) in enumerate(picked, start=1):
        H[b], f[b], lb[b], ub[b] = Hc, fc, lc, uc
    cnt = [_gi_iterations(H[b], f[b], lb[b], ub[b]) for b in range(5)]
    assert cnt[0] == (0, 1) and all(c[0] > 0 for c in cnt[1:]), cnt
    refs = [_oracle_box(H[b], f[b], lb[b], ub[b]) for b in range(5)]
    out = _solve_box(dev, monkeypatch, H, f, lb, ub)
    _check(out, refs)
    for path in PATHS:
        assert out[path][2].tolist() == [c[1] for c in cnt], (path, out[path][2], cnt)
    _check_loop(dev, H, f, lb, ub, refs)


# ----------------------------------------- four groups, four different states
@gpu
def test_four_states_in_one_wave(dev, monkeypatch):
    """One wave with a QP that settles at once, one that is cut at max_iter,
    one that is not convex and one that steps to its solution; then the same
    four and three more in two waves (a batch that is no multiple of four), in
    another order.  Every result equals, bit for bit, that of the QP alone."""
    n, cap = 20, 6
    rng = np.random.default_rng(8400)
    H, f, lb, ub = _random_problems(rng, n, 7)
    lb[np.isinf(lb)] = -1.5
    ub[np.isinf(ub)] = 1.5
    f[0] = 0.0                                               # settled
    H[1], f[1] = np.eye(n), np.where(np.arange(n) % 2, 20.0, -20.0)   # 20 iterations > cap
    H[2] = np.eye(n)
    H[2][3, 3] = -1.0                                        # not convex
    f[3] *= 0.05                                             # a few iterations
    its3 = _gi_iterations(H[3], f[3], lb[3], ub[3])[1]
    assert 0 < its3 <= cap, its3
    monkeypatch.delenv("MPCQP_KERNEL", raising=False)

    def run(idx):
        z, st = batched.solve_box(_t(_pack(H[idx]), dev), _t(f[idx], dev), _t(lb[idx], dev),
                                  _t(ub[idx], dev), max_iter=cap)
        torch.cuda.synchronize()
        return z.cpu().numpy(), st.cpu().numpy()

    alone = [run([i]) for i in range(7)]
    for idx in ([0, 1, 2, 3], [5, 3, 2, 6, 1, 0, 4]):
        z, st = run(idx)
        for k, i in enumerate(idx):
            assert np.array_equal(z[k], alone[i][0][0], equal_nan=True), (idx, i)
            assert st[k] == alone[i][1][0], (idx, i)
    code = [int(alone[i][1][0]) & 0xFF for i in range(4)]
    its = [(int(alone[i][1][0]) >> 8) & 0xFFFF for i in range(4)]
    assert code == [0, 1, 2, 0], code
    assert its[0] == 0 and its[1] in (cap, cap + 1) and its[3] == its3, its
    assert np.isnan(alone[2][0]).all() and np.array_equal(alone[0][0][0], np.zeros(n))
    z3 = _oracle_box(H[3], f[3], lb[3], ub[3])
    assert np.abs(alone[3][0][0] - z3).max() < TOL * max(1, np.abs(z3).max())


# ------------------------------------------------------------ every block size
@gpu
@pytest.mark.parametrize("n", [1, 4, 5, 8, 12, 20, 21, 32])
def test_every_block_size(dev, monkeypatch, n):
    """BS = 1, 1, 2, 2, 3, 5, 6, 8 (KB = 2 .. 5 index bits): five QPs with
    finite bounds, oracle, restated counts and comparator; the loop likewise."""
    batch = 5
    H, f, lb, ub = _random_problems(np.random.default_rng(8500 + n), n, batch)
    lb[np.isinf(lb)] = -1.0
    ub[np.isinf(ub)] = 1.0
    refs = [_oracle_box(H[b], f[b], lb[b], ub[b]) for b in range(batch)]
    want = [_gi_iterations(H[b], f[b], lb[b], ub[b])[1] for b in range(batch)]
    out = _solve_box(dev, monkeypatch, H, f, lb, ub)
    _check(out, refs)
    for path in PATHS:
        assert out[path][2].tolist() == want, (path, out[path][2], want)
    _check_loop(dev, H, f, lb, ub, refs)


@gpu
@pytest.mark.parametrize("N", [4, 5, 8, 12, 20, 21, 32])
def test_every_block_size_fused_step(dev, N):
    """mpcqp_mpc_box at the same sizes on the config-2 plant: oracle, and the
    iteration counts of the restatement on the oracle's condensed QP."""
    A, B, Q, R, Qf = _cfg2_plant()
    x0 = np.array([[8.0, -3.0], [0.0, 0.0], [-9.5, 6.5], [2.0, 1.5], [-4.0, 0.5]])
    batch = x0.shape[0]
    t = lambda a: _t(a, dev)  # noqa: E731
    refs, want = [], []
    for b in range(batch):
        d = oc.condense(A, B, Q, R, Qf, N, x0=x0[b])
        refs.append(_oracle_box(d["H"], d["f"], -np.ones(N), np.ones(N)))
        want.append(_gi_iterations(d["H"], d["f"], -np.ones(N), np.ones(N))[1])
    z, st = batched.mpc_box(t(np.broadcast_to(A, (batch, 2, 2))), t(np.broadcast_to(B, (batch, 2, 1))),
                            t(Q), t(R), t(Qf), N, t(x0), -1.0, 1.0)
    torch.cuda.synchronize()
    out = (z.cpu().numpy(), batched.status_code(st).cpu().numpy(), batched.status_iters(st).cpu().numpy())
    _check({"group": out}, refs, paths=("group",))
    assert out[2].tolist() == want, (out[2], want)


@gpu
def test_fp32_keeps_the_compare_and_select_reductions(dev, monkeypatch):
    """fp32 has no keyed reductions.  n = 22 (BS = 6), H = I, dyadic f with tied
    violations (the construction of test_scan_ties): the arithmetic is exact,
    so z, codes and counts equal the one-QP-per-wave kernel's bit for bit."""
    n, batch = 22, 6
    rng = np.random.default_rng(8600)
    f = rng.integers(-3, 4, (batch, n)) / 4.0
    for b in range(batch):
        rows = [(r + 3 * b) % n for r in (0, 1, 5, 6, 13, n - 1)]
        f[b, rows] = np.where(np.arange(len(rows)) % 2 == 0, -3.0, 3.0)
    H = np.broadcast_to(np.eye(n), (batch, n, n))
    t32 = lambda a: torch.as_tensor(np.array(a, dtype=np.float32), device=dev)  # noqa: E731
    res = {}
    for path in PATHS:
        if path == "wave":
            monkeypatch.setenv("MPCQP_KERNEL", "wave")
        else:
            monkeypatch.delenv("MPCQP_KERNEL", raising=False)
        z, st = batched.solve_box(t32(_pack(H)), t32(f), -1.0, 1.0)
        torch.cuda.synchronize()
        res[path] = (z.cpu().numpy(), st.cpu().numpy())
    monkeypatch.delenv("MPCQP_KERNEL", raising=False)
    assert res["group"][0].dtype == np.float32
    assert np.array_equal(res["group"][0], np.clip(-f, -1.0, 1.0).astype(np.float32))
    assert np.array_equal(res["group"][0], res["wave"][0])
    assert np.array_equal(res["group"][1], res["wave"][1])
    assert ((res["group"][1] >> 8) & 0xFFFF).tolist() == [6] * batch


# ------------------------------------------------------------- warm start
@gpu
@pytest.mark.parametrize("n,a", [(5, 1), (20, 6), (32, 9)])
def test_release_scan_tie(dev, n, a):
    """Three steps of the loop with H = I and bounds -1, 1.  Step 0 (f = -3 on
    rows a + 1 and n - 1, 0 elsewhere) puts those two rows on the upper bound in
    two iterations.  The shift hands step 1 three active rows: a, n - 2 and
    n - 1 (the last stage keeps its state).  Step 1 has f_a = 3/4 and f = 1/2 on
    rows n - 2 and n - 1: multipliers -(1 + f) = -7/4, -3/2 and -3/2, all of the
    wrong sign, exactly.  The release scan must drop a first, then, of the two
    equal ones, the smaller index.  With max_iter = 2 the third release is cut
    (MAXITER): row n - 2 is free and ends at -1/2, row n - 1 is still on its
    bound.  Without the cut all three end free.  Step 2 (f = 0) settles at 0.
    The same QPs in groups 0, 1 and 3 of the wave, zeros in group 2, and one
    more in a second wave."""
    batch = 5
    f0, f1 = np.zeros(n), np.zeros(n)
    f0[[a + 1, n - 1]] = -3.0
    f1[a], f1[n - 2], f1[n - 1] = 0.75, 0.5, 0.5
    fseq = np.stack([np.tile(f0, (batch, 1)), np.tile(f1, (batch, 1)), np.zeros((batch, n))])
    fseq[:, 2] = 0.0
    H = np.broadcast_to(np.eye(n), (batch, n, n))
    lb, ub = -np.ones((batch, n)), np.ones((batch, n))
    live = [0, 1, 3, 4]
    zs, code, its = _loop(dev, H, fseq, lb, ub, max_iter=2)
    print("cut:", code.tolist(), its.tolist())
    assert code[:, 2].tolist() == [0, 0, 0] and not zs[:, 2].any()
    for b in live:
        assert code[:, b].tolist() == [0, 1, 0], (b, code[:, b])
        assert np.array_equal(zs[0, b], np.clip(-f0, -1, 1)), b
        want = np.zeros(n)
        want[a], want[n - 2], want[n - 1] = -0.75, -0.5, 1.0
        assert np.array_equal(zs[1, b], want), (b, zs[1, b])
    zs, code, its = _loop(dev, H, fseq, lb, ub)
    assert (code == 0).all(), code
    for b in live:
        assert np.array_equal(zs[0, b], np.clip(-f0, -1, 1)), b
        assert np.array_equal(zs[1, b], -f1), (b, zs[1, b])
        assert not zs[2, b].any(), b
        # step 0: n sweeps + 2 iterations; step 1: n - 3 sweeps + 3 releases
        assert its[:2, b].tolist() == [n + 2, n], (b, its[:, b])
        shifted = _shifted(zs[0, b], lb[b], ub[b])
        assert np.flatnonzero(shifted).tolist() == [a, n - 2, n - 1]
        assert its[1, b] == _gi_iterations(np.eye(n), f1, lb[b], ub[b], warm=shifted)[1]
