"""Shared by tests/test_box_loop_vjp_host.py and tests/test_gpu_box_loop_vjp.py:
the NumPy closed form of the adjoint of the box-MPC loop
(mpcqp_mpc_box_loop_vjp) and the scenarios it is checked on.

Forward, per instance, t = 0..T-1:  f_t = F x_t + g_t,  z_t = argmin 1/2 z'Hz
+ f_t'z over lb <= z <= ub,  u_t = z_t[:nu],  x_{t+1} = A x_t + B u_t + w_t.
For a loss L(xs, us, zs) with upstream gradients gxs, gus, gzs:

    lam <- gxs[T]
    for t = T-1 .. 0:
        gz <- gzs[t];  gz[:nu] += gus[t] + B'lam
        d, nu, fold(d z_t') = the box-QP adjoint at z_t (_box_vjp_cases.closed_form)
        gg[t] = d, gw[t] = lam, gH += fold(d z_t'), gF += d x_t', gA += lam x_t',
        gB += lam u_t', glb += nu at lb, gub += nu at ub
        lam <- gxs[t] + A'lam + F'd
    gx0 = lam

The scenarios are those of _box_affine_cases.problem (per-instance plants and
bounds with +-inf and fixed entries, g and w; B = 5 instances, T = 6 steps) and
the loss is L = <c_x, xs> + <c_u, us> + <c_z, zs> with fixed standard-normal c.
"""
import numpy as np

import _box_affine_cases as ac
import _box_vjp_cases as vc
from oracle import condense as oc

MARGIN = 1e-3
SHAPES, FP32_SHAPES, B, T = ac.SHAPES, ac.FP32_SHAPES, ac.B, ac.T


def closed_form(A, Bm, H, F, lb, ub, xs, zs, gxs=None, gus=None, gzs=None):
    """One instance: dense H (n, n), xs (T+1, nx), zs (T, n), the upstream
    gradients in the same shapes (None = 0).  dict(gx0, gH (packed), gF, gA, gB,
    glb, gub, gg (T, n), gw (T, nx))."""
    steps, n = zs.shape
    nx, nu = Bm.shape
    lam = np.zeros(nx) if gxs is None else np.array(gxs[steps], float)
    o = dict(gH=np.zeros(n * (n + 1) // 2), gF=np.zeros((n, nx)), gA=np.zeros((nx, nx)),
             gB=np.zeros((nx, nu)), glb=np.zeros(n), gub=np.zeros(n), gg=np.zeros((steps, n)),
             gw=np.zeros((steps, nx)))
    for t in range(steps - 1, -1, -1):
        gz = np.zeros(n) if gzs is None else np.array(gzs[t], float)
        gz[:nu] += Bm.T @ lam + (0.0 if gus is None else gus[t])
        cf = vc.closed_form(H, zs[t], lb, ub, gz)
        d = cf["d"]
        o["gg"][t] = d
        o["gw"][t] = lam
        o["gH"] += cf["gH"]
        o["gF"] += np.outer(d, xs[t])
        o["gA"] += np.outer(lam, xs[t])
        o["gB"] += np.outer(lam, zs[t, :nu])
        o["glb"] += cf["glb"]
        o["gub"] += cf["gub"]
        lam = (0.0 if gxs is None else gxs[t]) + A.T @ lam + F.T @ d
    o["gx0"] = lam
    return o


def margin(H, F, lb, ub, xs, zs, g=None):
    """Non-degeneracy of an episode: the smallest, over the steps, of the active
    multipliers and the free rows' slack.  Fixed rows (lb == ub) are left out:
    their multiplier has no sign."""
    fixed = lb == ub
    vals = [np.inf]
    for t in range(zs.shape[0]):
        z = zs[t]
        kkt = H @ z + F @ xs[t] + (0.0 if g is None else g[t])
        at_lb, at_ub = vc.active_sets(z, lb, ub)
        if (at_lb & ~fixed).any():
            vals.append(kkt[at_lb & ~fixed].min())
        if (at_ub & ~fixed).any():
            vals.append((-kkt[at_ub & ~fixed]).min())
        free = ~(at_lb | at_ub)
        if free.any():
            vals.append(np.minimum(z[free] - lb[free], ub[free] - z[free]).min())
    return float(min(vals))


def weights(nx, nu, N):
    """The loss of a shape: c_x (T+1, B, nx), c_u (T, B, nu), c_z (T, B, n)."""
    rng = np.random.default_rng(777 + 100 * nx + 10 * nu + N)
    return (rng.standard_normal((T + 1, B, nx)), rng.standard_normal((T, B, nu)),
            rng.standard_normal((T, B, N * nu)))


def loss(c, i, xs, zs, nu):
    cx, cu, cz = c
    return float((cx[:, i] * xs).sum() + (cu[:, i] * zs[:, :nu]).sum() + (cz[:, i] * zs).sum())


def reference(nx, nu, N):
    """The closed form of every instance of problem(nx, nu, N) at the oracle's
    own episode, with the loss of weights(nx, nu, N)."""
    def make():
        p = ac.problem(nx, nu, N)
        cx, cu, cz = weights(nx, nu, N)
        out = []
        for i in range(B):
            d = p["cd"][i]
            xs, zs = p["ref"][i]
            out.append(closed_form(p["A"][i], p["B"][i], d["H"], d["F"], p["lb"][i], p["ub"][i],
                                   xs, zs, cx[:, i], cu[:, i], cz[:, i]))
        return out
    return ac.cached(("loop_vjp_reference", nx, nu, N), make)


# --------------------------------------- the weights of the condensed problem
def lower_matrix(gHp, n):
    """The gradient with respect to the lower triangle of H (what the packed
    entries are) as an (n, n) matrix with a zero upper triangle."""
    G = np.zeros((n, n))
    G[np.tril_indices(n)] = gHp
    return G


def weight_grads(Gam, Phi, gHp, gF, N, nx, nu):
    """dict(Q, R, Qf): the gradients of the shared weights from those of the
    condensed H = Gam' Qhat Gam + Rhat (packed lower) and F = Gam' Qhat Phi,
    symmetrised."""
    n = N * nu
    GL = lower_matrix(gHp, n)
    GQ = Gam @ GL @ Gam.T + Gam @ gF @ Phi.T
    blk = lambda M, k, w: M[k * w:(k + 1) * w, k * w:(k + 1) * w]  # noqa: E731
    return dict(Q=vc.sym(sum(blk(GQ, k, nx) for k in range(N - 1))) if N > 1 else np.zeros((nx, nx)),
                Qf=vc.sym(blk(GQ, N - 1, nx)), R=vc.sym(sum(blk(GL, k, nu) for k in range(N))))


FHC_N, FHC_T, FHC_B = 8, 6, 5


def fhc_episode():
    """The FHC double integrator (|u| <= 1, N = 8, T = 6), five initial states
    with mixed active sets: dict(A, B, Q, R, Qf, cd, x0, lb, ub, c, ref = the
    oracle's (xs, zs) per instance)."""
    def make():
        A, Bm, Q, R, Qf = ac.fhc_plant()
        # the seed at which the oracle's episodes are furthest from degenerate
        # (margin 1.4e-2) among the first dozen, with 2 % .. 94 % of the rows active
        rng = np.random.default_rng(7)
        x0 = rng.uniform(-3.0, 3.0, (FHC_B, 2))
        lb, ub = -np.ones(FHC_N), np.ones(FHC_N)
        cd = oc.condense(A, Bm, Q, R, Qf, FHC_N)
        c = (rng.standard_normal((FHC_T + 1, FHC_B, 2)), rng.standard_normal((FHC_T, FHC_B, 1)),
             rng.standard_normal((FHC_T, FHC_B, FHC_N)))
        ref = [ac.host_loop(A, Bm, cd["H"], cd["F"], lb, ub, x0[i], FHC_T) for i in range(FHC_B)]
        return dict(A=A, B=Bm, Q=Q, R=R, Qf=Qf, cd=cd, x0=x0, lb=lb, ub=ub, c=c, ref=ref)
    return ac.cached("loop_vjp_fhc", make)


def fhc_weight_grads(p, i, xs=None, zs=None):
    """dict(Q, R, Qf, x0, glb, gub) of instance i of fhc_episode() by the closed
    form and the mapping, at the oracle's episode or at the given one."""
    cd = p["cd"]
    if xs is None:
        xs, zs = p["ref"][i]
    cx, cu, cz = p["c"]
    cf = closed_form(p["A"], p["B"], cd["H"], cd["F"], p["lb"], p["ub"], xs, zs, cx[:, i],
                     cu[:, i], cz[:, i])
    o = weight_grads(cd["Gam"], cd["Phi"], cf["gH"], cf["gF"], FHC_N, 2, 1)
    o.update(x0=cf["gx0"], glb=cf["glb"], gub=cf["gub"])
    return o
