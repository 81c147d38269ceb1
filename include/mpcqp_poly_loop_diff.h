/*
 * mpcqp_poly_loop_diff.h -- the adjoint of the one-launch state-constrained
 * MPC loop (mpcqp_mpc_poly_loop and mpcqp_mpc_poly_loop_affine of mpcqp.h),
 * next to the C ABI of mpcqp.h, mpcqp_diff.h and mpcqp_poly_diff.h (same
 * library, same MPCQP_ABI_VERSION).
 *
 * The reference (konnpaku-youmu/Model_Predictive_Control) runs its
 * state-constrained MPC in closed loop (session_2/3: simulate(...) around an
 * IPOPT plan per step) and never differentiates the trajectory; a loss on such
 * an episode reaches x0, the disturbances, the per-step linear terms and row
 * shifts, the row bounds, the box, the cost, the rows and the plant through
 * mpcqp_mpc_poly_loop_vjp, as a loss on an input-box episode does through
 * mpcqp_mpc_box_loop_vjp.
 *
 * Conventions: those of mpcqp.h and mpcqp_poly_diff.h, all of them.
 *  - dtype: MPCQP_F64 or MPCQP_F32; every floating buffer of a call has it.
 *  - Buffers are caller-owned DEVICE pointers, row-major, step-outermost, then
 *    batch.  The library keeps no pointer after the call returns.
 *  - stream is a hipStream_t (NULL = default stream).  Calls only enqueue
 *    work; they never synchronise, allocate or free (graph-capturable).
 *  - Return value: MPCQP_OK (0) or a negative error code; the message is
 *    available from mpcqp_last_error() (thread-local).
 */
#ifndef MPCQP_POLY_LOOP_DIFF_H
#define MPCQP_POLY_LOOP_DIFF_H

#include <stddef.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of `scratch` mpcqp_mpc_poly_loop_vjp needs when gzs is given: the
 * products Hinv gzs (steps x batch x n) and Ut gzs (steps x batch x m_total),
 * each aligned to 256 bytes.  0 for sizes the call itself refuses.
 */
size_t mpcqp_mpc_poly_loop_vjp_workspace(int dtype, int batch, int n, int m, int nbox, int steps);

/*
 * Adjoint (vector-Jacobian product) of a whole episode of mpcqp_mpc_poly_loop
 * or mpcqp_mpc_poly_loop_affine.  The forward, per instance and step
 * t = 0..steps-1, with C = [G; I] (m_total = m + (nbox ? n : 0) rows):
 *
 *     z_t = argmin 1/2 z'Hz + (F x_t + g_t)'z
 *           s.t.  hl - E x_t - e_t <= G z <= hu - E x_t - e_t,  lbz <= z <= ubz
 *     u_t = z_t[0..nu),   x_{t+1} = A x_t + B u_t + w_t
 *
 * with y_t the signed multipliers, an exact 0 on every inactive row.  From the
 * upstream gradients gxs = dL/dxs ((steps+1) x batch x nx), gus = dL/dus
 * (steps x batch x nu), gzs = dL/dzs (steps x batch x n) and gys = dL/dys
 * (steps x batch x m_total), each of which may be NULL (= 0), and the shared
 * factors the setup left in `workspace`:
 *
 *     lam <- gxs[steps]
 *     for t = steps-1 .. 0:
 *         v     = gus[t] + B'lam;   gz = gzs[t],  gz[0..nu) += v
 *         A_t   = {i : ys[t]_i != 0}
 *         r     = Ut gz,   q = Hinv gz
 *         eps_t = M_AA^{-1} (r_A - gys[t]_A) on A_t, 0 elsewhere
 *         gf[t] = dL/dg_t = -(q - Ut_A' eps_A)                         (n)
 *         gw[t] = dL/dw_t = lam                                        (nx)
 *         ghu_i += eps_t,i where ys[t]_i > 0,  ghl_i += eps_t,i where ys[t]_i < 0
 *         lam  <- gxs[t] + A'lam + Kt gz - L_A' eps_A - E' eps_t[0..m)
 *     gx0 = lam
 *
 * Outputs, each may be NULL except vstatus: gx0 (batch x nx); ghl, ghu (batch x
 * m_total, summed over the episode; the entries m.. are the instance's dL/dlbz
 * and dL/dubz); geps (steps x batch x m_total, the rows eps_t: dL/de_t is
 * -geps[t][0..m)); gf (steps x batch x n); gw (steps x batch x nx).  Without
 * gf the call does no n-wide work (beyond Kt gzs[t] when gzs is given).
 * Gradients of the shared operands are left to the caller, as sums over all
 * (t, b) rows: with S = sum gf_t z_t', dL/dH on the packed entries is
 * (i, j<i) = S_ij + S_ji, (i, i) = S_ii; dL/dF = sum gf_t x_t'; dL/dG = the rows
 * < m of sum (y_t gf_t' - eps_t z_t'); dL/dE = -sum eps_t[0..m) x_t';
 * dL/dA = sum gw_t x_t'; dL/dB = sum gw_t u_t'.
 *
 * A row that sits at its bound with y = 0 counts as inactive, as in
 * mpcqp_poly_solve_vjp.  Every step is rebuilt from M and swept on the rows of
 * A_t in ascending order: on the same ys[t], gzs[t], gys[t] a step's eps_t and
 * gf[t] are those of mpcqp_poly_solve_vjp bit for bit.
 *
 * Inputs: workspace as mpcqp_poly_setup wrote it for the same (dtype, n, m,
 * nbox, nx), read-only; E (m x nx, or NULL), A (nx x nx) and Bm (nx x nu) as
 * given to the forward, shared by the batch; ys (steps x batch x m_total,
 * required for steps > 0) and status (steps x batch; NULL: every step counts
 * as OPTIMAL) as the forward wrote them.  scratch:
 * mpcqp_mpc_poly_loop_vjp_workspace bytes, needed when gzs is given and
 * steps > 0; a smaller one is MPCQP_EINVAL.  Without gzs there is one launch
 * and no scratch; with it the products Hinv gzs and Ut gzs of all steps are one
 * launch of mpcqp_mpc_poly_loop_affine's preparation before it.
 *
 * vstatus[b] (required) is a bare MPCQP_STATUS_* code, the first of
 *   1. the code of the earliest step whose status word is not plainly
 *      OPTIMAL: its low byte if that is not OPTIMAL (MAXITER included), else
 *      INFEASIBLE if the word carries MPCQP_STATUS_SOFTENED -- a step of
 *      mpcqp_mpc_poly_loop_soft that ended with a slack did not satisfy the
 *      hard rows this adjoint differentiates;
 *   2. NOT_CONVEX if the setup found H not positive definite (every instance);
 *   3. NONFINITE if ys, a given upstream gradient or the instance's rows of
 *      Hinv gzs or Ut gzs hold a NaN or Inf, at any step;
 *   4. NOT_CONVEX if at any step a pivot of the solve with M_AA is not above
 *      tol * max(M_kk, 1e-300), tol = 1e-10 (fp64) or 1e-5 (fp32), the
 *      dependence test of the forward;
 *   5. OPTIMAL.
 * Where vstatus[b] is not OPTIMAL every output of that instance is an exact
 * zero, all its rows of geps, gf and gw included; the other instances are not
 * affected.  steps == 0 gives gx0 = gxs[0] and zeros in ghl, ghu.
 *
 * One instance per wavefront, the whole reverse episode in one launch.  No
 * atomics; every sum has a fixed order, so a replay gives identical bits.
 * Division is the reciprocal of the forward (loop_poly.hip), not IEEE.
 *
 * Limits: those of mpcqp_mpc_poly_loop, m_total in [1, 64], 1 <= nx <= 16,
 * 1 <= nu <= min(16, n) (MPCQP_EINVAL outside them); batch == 0 returns
 * MPCQP_OK.
 * Not supported: the soft variant (mpcqp_mpc_poly_loop_soft: see rule 1);
 * per-instance A, B or E; sweeps carried from one step to the next (every
 * step costs |A_t| sweeps); second derivatives.
 */
int mpcqp_mpc_poly_loop_vjp(int dtype, int batch, int n, int m, int nbox, int nx, int nu,
                            int steps,
                            const void* workspace, const void* E, const void* A, const void* Bm,
                            const void* ys, const int32_t* status,
                            const void* gxs, const void* gus, const void* gzs, const void* gys,
                            void* gx0, void* ghl, void* ghu, void* geps, void* gf, void* gw,
                            int32_t* vstatus,
                            void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_POLY_LOOP_DIFF_H */
