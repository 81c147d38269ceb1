"""CPU: the closed form of the box-QP adjoint (tests/_box_vjp_cases.py) against
central differences of the oracle's active set, and the argument checks of
mpcqp_solve_box_vjp, which run before any device work.

Central differences with eps = 1e-6 on 32 instances per shape, L = g.z with a
fixed standard-normal g.  Worst disagreement relative to 1 + max|grad| of the
instance: 3.9e-11, 1.1e-10, 1.1e-8, 3.8e-8, 1.9e-7 at n = 1, 5, 17, 20, 32 (it
grows with cond(H), 4.4e4 at n = 32: the round-off of the differences) and
5.4e-10 on the random nx = 3, nu = 2, N = 4 plant; no instance is degenerate
(margin 1e-3).  The bound is 1e-6.  Each parameter group is also held against
1 + its own max|grad|, with max(1e-6, eps_mach cond(H) / (2 eps)): 1e-6 up to
n = 20 and 4.9e-6 at n = 32, where the differences' round-off alone reaches
1.9e-6 on a group."""
import ctypes

import numpy as np
import pytest

import _box_vjp_cases as vc
from model_predictive_control_amd import _native as nat
from oracle import condense as oc
from oracle import qp as oq

EPS = 1e-6
TOL = 1e-6  # relative to 1 + max|grad|
MAX_DROPPED = 2


def _loss(p, i, **over):
    """L = g.z* of instance i with some of f, lb, ub, x0, Q, R, Qf replaced."""
    H, f = p["H"][i], p["f"][i]
    if any(k in over for k in ("x0", "Q", "R", "Qf")):
        cd = oc.condense(p["A"], p["B"], over.get("Q", p["Q"]), over.get("R", p["R"]),
                         over.get("Qf", p["Qf"]), p["N"], x0=over.get("x0", p["x0"][i]))
        H, f = cd["H"], cd["f"]
    z = oq.box_qp(H, over.get("f", f), over.get("lb", p["lb"][i]), over.get("ub", p["ub"][i]))[0]
    return float(p["g"][i] @ z)


def _fd_vector(p, i, name, x):
    out = np.zeros(x.size)
    for k in range(x.size):
        e = np.zeros(x.size)
        e[k] = EPS
        out[k] = (_loss(p, i, **{name: x + e}) - _loss(p, i, **{name: x - e})) / (2 * EPS)
    return out


def _fd_weight(p, i, name, W):
    """<dL/dW, E> for the symmetric directions E = e_i e_j' + e_j e_i' (i < j)
    and e_i e_i', as an upper-triangular list."""
    k = W.shape[0]
    out = []
    for a in range(k):
        for b in range(a, k):
            E = np.zeros((k, k))
            E[a, b] = E[b, a] = EPS
            out.append((_loss(p, i, **{name: W + E}) - _loss(p, i, **{name: W - E})) / (2 * EPS))
    return np.array(out)


def _weight_dirs(G):
    """The same directional derivatives from the symmetrised gradient G."""
    k = G.shape[0]
    return np.array([G[a, b] if a == b else 2 * G[a, b] for a in range(k) for b in range(a, k)])


def _check_batch(p):
    worst, dropped, worst_group = 0.0, 0, 0.0
    # round-off of a central difference of the oracle: eps_mach cond(H) / (2 EPS)
    # (6.6e-7 at n = 20, 4.9e-6 at n = 32; H is the same for a whole batch)
    roundoff = np.finfo(float).eps * np.linalg.cond(p["H"][0]) / (2 * EPS)
    for i in range(p["x0"].shape[0]):
        if not p["nondeg"][i]:
            dropped += 1
            continue
        cf = vc.closed_form(p["H"][i], p["z"][i], p["lb"][i], p["ub"][i], p["g"][i])
        mg = vc.mpc_grads(p["cd"][i], p["z"][i], cf["d"], p["N"], p["nx"], p["nu"])
        pairs = [(cf["d"], _fd_vector(p, i, "f", p["f"][i])),
                 (cf["glb"], _fd_vector(p, i, "lb", p["lb"][i])),
                 (cf["gub"], _fd_vector(p, i, "ub", p["ub"][i])),
                 (mg["x0"], _fd_vector(p, i, "x0", p["x0"][i])),
                 (_weight_dirs(mg["Q"]), _fd_weight(p, i, "Q", p["Q"])),
                 (_weight_dirs(mg["R"]), _fd_weight(p, i, "R", p["R"])),
                 (_weight_dirs(mg["Qf"]), _fd_weight(p, i, "Qf", p["Qf"]))]
        # One scale per instance, 1 + the largest gradient entry of any of its
        # parameters: the round-off of a central difference is an absolute
        # error of the loss, eps_mach cond(H) |z| / EPS, whichever parameter moved.
        scale = 1 + max(float(np.abs(an).max()) for an, _ in pairs)
        for an, fd in pairs:
            worst = max(worst, float(np.abs(an - fd).max()) / scale)
            # Each group also against its own scale, so that a group of small
            # entries is not hidden behind the instance's largest: the same
            # TOL, raised only where that round-off exceeds it (n = 32).
            group = float(np.abs(an - fd).max()) / (1 + float(np.abs(an).max()))
            worst_group = max(worst_group, group / max(TOL, roundoff))
    return worst, dropped, worst_group


@pytest.mark.parametrize("n", vc.SIZES)
def test_closed_form_vs_central_differences_session1(n):
    p = vc.session1_batch(n)
    worst, dropped, group = _check_batch(p)
    print(f"n={n}: worst relative disagreement {worst:.2e}, dropped {dropped}, "
          f"per group {group:.2f} of its bound")
    assert dropped <= MAX_DROPPED, dropped
    assert worst <= TOL, worst
    assert group <= 1.0, group


def test_closed_form_vs_central_differences_random_plant():
    p = vc.random_batch()
    on = (p["z"] == p["lb"]) | (p["z"] == p["ub"])
    assert on.any() and (~on).any()
    worst, dropped, group = _check_batch(p)
    print(f"random plant: worst relative disagreement {worst:.2e}, dropped {dropped}, "
          f"per group {group:.2f} of its bound")
    assert dropped <= MAX_DROPPED, dropped
    assert worst <= TOL, worst
    assert group <= 1.0, group


def test_h_gradient_vs_central_differences():
    """dL/dH folded onto the packed entries, on the n = 5 cases: packed entry
    (i, j) moves H_ij and H_ji together."""
    p = vc.session1_batch(5)
    r, c = np.tril_indices(5)
    for i in vc.nondegenerate(p, 4):
        cf = vc.closed_form(p["H"][i], p["z"][i], p["lb"][i], p["ub"][i], p["g"][i])
        fd = np.zeros(r.size)
        for k in range(r.size):
            E = np.zeros((5, 5))
            E[r[k], c[k]] = E[c[k], r[k]] = EPS
            lp = p["g"][i] @ oq.box_qp(p["H"][i] + E, p["f"][i], p["lb"][i], p["ub"][i])[0]
            lm = p["g"][i] @ oq.box_qp(p["H"][i] - E, p["f"][i], p["lb"][i], p["ub"][i])[0]
            fd[k] = (lp - lm) / (2 * EPS)
        assert np.abs(cf["gH"] - fd).max() <= TOL * (1 + np.abs(fd).max())


def test_fixture_cases_are_nondegenerate(golden):
    """The 64 config-2 fixtures the GPU test compares on: at most 2 degenerate."""
    g = golden("boxqp_cfg2.npz")
    n = g["f"].shape[1]
    lb, ub = -np.ones(n), np.ones(n)
    m = np.array([vc.margin(g["H"][i], g["f"][i], lb, ub, g["z"][i]) for i in range(g["z"].shape[0])])
    assert g["z"].shape[0] == 64 and (m <= vc.MARGIN).sum() <= 2, np.sort(m)[:4]


# ------------------------------------------------------------------- the ABI
def _call(lib, *, dtype=nat.F64, batch=4, n=20, ptr=True):
    """mpcqp_solve_box_vjp with dummy pointers (never dereferenced: every call
    here fails in the argument checks or has batch = 0)."""
    one = ctypes.c_void_p(1) if ptr else None
    return lib.mpcqp_solve_box_vjp(dtype, batch, n, one, 0, one, None, 0, None, 0, None, one,
                                   one, None, None, None, None, None)


def test_symbol_and_argument_checks():
    lib = nat.load()
    assert hasattr(lib, "mpcqp_solve_box_vjp")
    assert "mpcqp_solve_box_vjp" in nat.SIGNATURES
    err = lib.mpcqp_last_error
    assert _call(lib, dtype=7) == -1 and b"dtype" in err()
    assert b"mpcqp_solve_box_vjp" in err()
    assert _call(lib, n=33) == -3 and b"32" in err()
    assert _call(lib, n=0) == -1
    assert _call(lib, batch=-1) == -1
    assert _call(lib, batch=0) == 0
    assert _call(lib, batch=0, ptr=False) == 0
    assert _call(lib, ptr=False) == -1 and b"required" in err()
