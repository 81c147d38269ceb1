/*
 * mpcqp_poly_diff.h -- the adjoint of the stand-alone polytope QP
 * (mpcqp_poly_setup / mpcqp_poly_solve of mpcqp.h), next to the C ABI of
 * mpcqp.h and mpcqp_diff.h (same library, same MPCQP_ABI_VERSION).
 *
 * The reference (konnpaku-youmu/Model_Predictive_Control) hands its
 * state-constrained plans to IPOPT (session_2/3: the state box on x_1..x_N,
 * session_4/main.py:115-116) and never differentiates them; a loss on such a
 * plan reaches x0, the row bounds, the box, the cost and the rows through
 * mpcqp_poly_solve_vjp, as a loss on an input-box plan does through
 * mpcqp_solve_box_vjp.
 *
 * Conventions: those of mpcqp.h, all of them.
 *  - dtype: MPCQP_F64 or MPCQP_F32; every floating buffer of a call has it.
 *  - Buffers are caller-owned DEVICE pointers, row-major, batch-outermost.
 *    The library keeps no pointer after the call returns.
 *  - stream is a hipStream_t (NULL = default stream).  Calls only enqueue
 *    work; they never synchronise, allocate or free (graph-capturable).
 *  - Return value: MPCQP_OK (0) or a negative error code; the message is
 *    available from mpcqp_last_error() (thread-local).
 */
#ifndef MPCQP_POLY_DIFF_H
#define MPCQP_POLY_DIFF_H

#include <stddef.h>

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of `scratch` mpcqp_poly_solve_vjp needs when gz is given: the products
 * Hinv gz (batch x n) and Ut gz (batch x m_total), each aligned to 256 bytes.
 * 0 for sizes the call itself refuses.
 */
size_t mpcqp_poly_solve_vjp_workspace(int dtype, int batch, int n, int m, int nbox);

/*
 * Adjoint (vector-Jacobian product) of mpcqp_poly_solve at its optimum.  The
 * forward, per instance, with C = [G; I] (m_total = m + (nbox ? n : 0) rows)
 * and f = F x0 + f1:
 *
 *     z = argmin 1/2 z'Hz + f'z   s.t.  hl <= G z <= hu,  lbz <= z <= ubz
 *
 * with the signed multipliers y (> 0 at the upper side, < 0 at the lower).
 * The forward writes y as an exact 0 on every inactive row, so the active set
 * is  A = {i : y_i != 0}  and the side is the sign of y_i.  From the upstream
 * gradients gz = dL/dz (batch x n) and gy = dL/dy (batch x m_total; only its
 * active entries matter), each of which may be NULL (= 0), and the shared
 * factors the setup left in `workspace` (Hinv, Ut = C Hinv, M = C Hinv C',
 * Kt = (-Hinv F)', L = -Ut F):
 *
 *     q   = Hinv gz,   r = Ut gz
 *     e_A = M_AA^{-1} (r_A - gy_A),   e = 0 elsewhere
 *     gf  = dL/df1 = -(q - Ut_A' e_A)                       (n)
 *     gx0 = dL/dx0 = F' gf = Kt gz - L_A' e_A               (nx)
 *     ghu_i = e_i where y_i > 0,  ghl_i = e_i where y_i < 0,  0 elsewhere
 *
 * ghl and ghu cover all m_total rows: the entries m.. are dL/dlbz and dL/dubz
 * of the instance.  Outputs are per instance and dense, each may be NULL: gf
 * (batch x n), gx0 (batch x nx, needs nx > 0 and a setup with F), ghl, ghu
 * (batch x m_total).  Gradients of the shared operands are left to the caller:
 * with S = sum_b gf_b z_b',  dL/dH on the packed entries is (i, j<i) = S_ij +
 * S_ji, (i, i) = S_ii (as mpcqp_solve_box_vjp folds it), dL/dF = sum_b gf_b
 * x0_b', dL/dG = the rows < m of sum_b (y_b gf_b' - e_b z_b') with e = ghl +
 * ghu, and dL/dlbz, dL/dubz the batch sums of the rows m.. of ghl and ghu.
 *
 * A row that sits at its bound with y_i == 0 counts as inactive: the result is
 * the one-sided derivative on the side that lets the row leave, which is how
 * the forward's own epilogue treats it.  With m = 0 the formulas are those of
 * mpcqp_solve_box_vjp (gf = d, e = nu on the side held).
 *
 * Inputs: workspace as mpcqp_poly_setup wrote it for the same (dtype, n, m,
 * nbox, nx), read-only; y (batch x m_total) and status (batch) as
 * mpcqp_poly_solve wrote them; status may be NULL (every instance OPTIMAL).
 * scratch: mpcqp_poly_solve_vjp_workspace bytes, needed when gz is given; a
 * smaller one is MPCQP_EINVAL.
 *
 * vstatus[b] (required) is a bare MPCQP_STATUS_* code, decided in this order:
 *   1. the low byte of status[b] if that is not OPTIMAL (MAXITER included);
 *   2. else NOT_CONVEX if the setup found H not positive definite (every
 *      instance);
 *   3. else NONFINITE if y, gz, gy or the instance's rows of q or r hold a
 *      NaN or Inf;
 *   4. else NOT_CONVEX if a pivot of the solve with M_AA is not above
 *      tol * max(M_kk, 1e-300), tol = 1e-10 (fp64) or 1e-5 (fp32), the
 *      dependence test of the forward: the rows marked active are dependent
 *      and the gradient is not defined;
 *   5. else OPTIMAL.
 * Where vstatus[b] is not OPTIMAL every output of that instance is an exact
 * zero; the other instances are not affected.
 *
 * Two launches.  The product q, r for all instances is the skinny GEMM of
 * mpcqp_mpc_poly_loop_affine's preparation (an element of Hinv or Ut is loaded
 * once per 16 instances).  The adjoint proper runs one instance per wavefront:
 * M swept on the rows of A in ascending order (|A| sweeps) on the register
 * grid of the forward, one mat-vec, and the forward's epilogue loop for gf.
 * No atomics; every sum has a fixed order, so a replay gives identical bits.
 * Division is the reciprocal of the forward (solve_poly.hip), not IEEE.
 *
 * Limits: those of mpcqp_poly_solve, m_total in [1, 64] and nx <= 16
 * (MPCQP_EINVAL outside them); batch == 0 returns MPCQP_OK.
 * Not supported: mpcqp_solve_qp, second derivatives.  (The adjoint of
 * mpcqp_mpc_poly_loop and its affine variant is mpcqp_mpc_poly_loop_vjp of
 * mpcqp_poly_loop_diff.h; the soft variant has none.)
 */
int mpcqp_poly_solve_vjp(int dtype, int batch, int n, int m, int nbox, int nx,
                         const void* workspace, const void* y, const int32_t* status,
                         const void* gz, const void* gy,
                         void* gf, void* gx0, void* ghl, void* ghu,
                         int32_t* vstatus,
                         void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_POLY_DIFF_H */
