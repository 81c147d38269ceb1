/*
 * mpcqp_diff.h -- the differentiable-condensing entry point of libmpcqp.so,
 * next to the C ABI of mpcqp.h (same library, same MPCQP_ABI_VERSION).
 *
 * The reference (konnpaku-youmu/Model_Predictive_Control) builds its OCP by
 * symbolic single shooting (session_4/main.py:86-106) and never differentiates
 * it with respect to the model; mpcqp_condense_vjp is what model learning and
 * system identification through the controller need on top of
 * mpcqp_solve_box_vjp and mpcqp_mpc_box_loop_vjp, which stop at dL/dH, dL/dF
 * and dL/df.
 *
 * Conventions: those of mpcqp.h, all of them.
 *  - dtype: MPCQP_F64 or MPCQP_F32; every floating buffer of a call has it.
 *  - Buffers are caller-owned DEVICE pointers, row-major, batch-outermost.  A
 *    "stride" is the element distance between consecutive instances; stride 0
 *    means one buffer shared by the batch.  The library keeps no pointer after
 *    the call returns.
 *  - z is stage-major: z = [u_0; u_1; ...; u_{N-1}].
 *  - Symmetric n x n matrices are stored PACKED LOWER, row-major: element
 *    (i, j<=i) at i*(i+1)/2 + j, n(n+1)/2 per instance.
 *  - stream is a hipStream_t (NULL = default stream).  Calls only enqueue
 *    work; they never synchronise, allocate or free (graph-capturable).
 *  - Return value: MPCQP_OK (0) or a negative error code; the message is
 *    available from mpcqp_last_error() (thread-local).
 */
#ifndef MPCQP_DIFF_H
#define MPCQP_DIFF_H

#include "mpcqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Adjoint (vector-Jacobian product) of mpcqp_condense: from the gradients of a
 * loss with respect to the condensed problem, gH (dL/dH on the packed entries,
 * n(n+1)/2: entry (i, j<i) carries both halves, as mpcqp_solve_box_vjp and
 * mpcqp_mpc_box_loop_vjp write it), gF (dL/dF, n x nx) and gf (dL/df, n), each
 * per instance and dense and each of which may be NULL (= 0), the gradients
 * with respect to everything mpcqp_condense takes.  n = N*nu.
 *
 * Let Ghat be the symmetric n x n matrix with Ghat_ii = gH_ii and Ghat_ij =
 * Ghat_ji = gH_ij / 2, GY = [Ghat, gF, gf] (n x (n+nx+1)), and S the stacked
 * block rows  S_k = [Gam_k, Phi_k, xbar_k]  (nx x (n+nx+1)) of the forward:
 *
 *   S_{-1} = [0, I, x0],   S_k = A_k S_{k-1} + E_k,   E_k = [B_k in column
 *   block k, 0, c_k],      [H - Rhat, F, f] = sum_k Gam_k' Q_k S_k,
 *   Q_k = Q for k < N-1 and Qf for k = N-1.
 *
 *   for k = N-1 .. 0:
 *     T_k   = Gam_k GY S_k'                    gQf = T_{N-1},  gQ = sum_{k<N-1} T_k
 *     GS_k  = Q_k' Gam_k GY;   GS_k[:, 0..n) += Q_k S_k GY'
 *     Lam_k = GS_k + A_{k+1}' Lam_{k+1}        (Lam_N = 0)
 *     gA_k  = Lam_k S_{k-1}'   gB_k = Lam_k[:, k*nu..(k+1)*nu)   gc_k = Lam_k[:, last]
 *   gx0 = (A_0' Lam_0)[:, last]                gR = sum_k Ghat[k*nu.., k*nu..]
 *
 * Without MPCQP_TV gA and gB are summed over k.  gQ, gQf and gR are returned
 * symmetrised, (M + M')/2.
 * Inputs: exactly those of mpcqp_condense (per-instance strides in elements, 0
 * = shared; c and x0 optional, NULL = 0).  flags is 0 or MPCQP_TV; any other
 * bit, MPCQP_GAM_PACKED included, is MPCQP_EINVAL.  A, Bm, Q, R, Qf are
 * required.
 * Outputs, per instance and dense, each may be NULL: gA (nx*nx, or N*nx*nx
 * with MPCQP_TV), gB (nx*nu, or N*nx*nu), gQ (nx*nx), gR (nu*nu), gQf (nx*nx),
 * gc (N*nx, valid also when c is NULL), gx0 (nx), vstatus (batch).  Gradients
 * of shared inputs are left to the caller to sum.
 * vstatus[b] is a bare MPCQP_STATUS_* code: NONFINITE if any input of the
 * instance (A, Bm, Q, R, Qf, c, x0) or any given upstream row (gH, gF, gf)
 * holds a NaN/Inf, else OPTIMAL.  Where it is NONFINITE every output of that
 * instance is an exact zero; the other instances are not affected.
 * One instance per wavefront: lane j owns column j of S_k, Lam_k and GY; the
 * block rows S_k of a forward pass and GY stay in LDS; the sums over the
 * columns (gQ, gQf, gA) are taken once, after the recursion, in lane order.
 * No atomics and no scratch: every sum has a fixed order, so a replay gives
 * identical bits, and the call only enqueues on `stream` and allocates
 * nothing.
 * Limits: nx <= 4, nu <= 2, N*nu <= 32, those of every differentiable path
 * (MPCQP_ENOTSUP above them inside the limits of mpcqp_condense, with the
 * limit in mpcqp_last_error(); MPCQP_EINVAL outside mpcqp_condense's own);
 * batch == 0 returns MPCQP_OK.
 * Not supported: a gradient input for Gam, Phi or xbar (reference tracking
 * builds its linear term from Gam), second derivatives.
 */
int mpcqp_condense_vjp(int dtype, int batch, int nx, int nu, int N, int flags,
                       const void* A, int64_t strideA, const void* Bm, int64_t strideB,
                       const void* Q, int64_t strideQ, const void* R, int64_t strideR,
                       const void* Qf, int64_t strideQf, const void* c, int64_t strideC,
                       const void* x0, int64_t strideX0,
                       const void* gH, const void* gF, const void* gf,
                       void* gA, void* gB, void* gQ, void* gR, void* gQf, void* gc, void* gx0,
                       int32_t* vstatus, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MPCQP_DIFF_H */
