// mpc_factor.hpp -- -H^{-1} of the condensed input-box OCP from the factors
// the Riccati pass already holds (used by mpc_group_kernel, quad_box.hip).
//
// With x_0 = 0 and no drift, completing the square stage by stage gives
//     J(u) = sum_k (u_k - K_k x_k)' S_k (u_k - K_k x_k),  S_k = R + B_k'P_{k+1}B_k,
// so H = T' diag(S_k) T with T the unit lower block-triangular map u -> v,
// v_k = u_k - K_k x_k(u), and
//     H^{-1} = W diag(S_k^{-1}) W',   W = T^{-1}.
// Column (j, b) of W is a closed-loop rollout started at stage j:
//     u_j = e_b, x_{j+1} = B_j e_b;   u_k = K_k x_k, x_{k+1} = (A_k + B_k K_k) x_k  (k > j),
// zero before stage j.  With S_k^{-1} = L_k L_k' (Cholesky) the rollout is
// started from u_j = L_j[:, b] instead, which yields column (j, b) of
// W~ = W diag(L_k), and -H^{-1} = -W~ W~' is a plain Gram product.
//
// Row form.  A column needs K_j .. K_{N-1}, so the rollouts cannot start
// before the backward Riccati pass has ended.  The same matrix by rows,
// backward in the column stage j, runs in lockstep with that pass:
//     W~[(t,a), (j,:)] = Psi_j(t)[a, :] B_j L_j   (t > j),    L_j[a, :]  (t = j),    0  (t < j),
//     Psi_j(t) := K_t Acl_{t-1} ... Acl_{j+1},    Acl_k = A_k + B_k K_k,
//     Psi_{j-1}(t) = Psi_j(t) Acl_j,              Psi_{j-1}(j) = K_j,
// which is the column formula read along t: u_t = K_t x_t with
// x_t = Acl_{t-1} ... Acl_{j+1} B_j L_j[:, b].  The state of row (t, a) is the
// 1 x NX vector Psi_j(t)[a, :]; it is 0 until step j = t sets it to K_t[a, :],
// so the rows t < j come out 0 by themselves.
//
// f in the same loop.  The adjoint y_k = Q xbar_k + A_k'y_{k+1}, y_N = Qf xbar_N,
// f_k = B_k'y_{k+1} needs xbar_k for descending k, hence all of xbar first.
// With y_k = Pi_k xbar_k + pi_k and xbar_{k+1} = A_k xbar_k + c_k it becomes
//     Pi_k = Q + A_k' Pi_{k+1} A_k,   pi_k = A_k'(Pi_{k+1} c_k + pi_{k+1}),   Pi_N = Qf, pi_N = 0,
//     f_k = (B_k' Pi_{k+1}) xbar_{k+1} + B_k' pi_{k+1},
// a backward recursion that does not depend on x0 (pi = 0 without a drift):
// the row (k, a) keeps (B_k' Pi_{k+1})[a, :] from backward step k and
// xbar_{k+1} from forward step k (quad_box.hip, row form).
#pragma once
#include "common.hpp"

namespace mpcqp {

// Column b of the lower Cholesky factor of the symmetric positive definite
// NU x NU matrix Si (row-major, NU <= 2).  A non-positive pivot gives NaN; the
// Riccati pass has flagged that instance NOT_CONVEX already.
template <typename T, int NU>
__device__ __forceinline__ void chol_col(const T* Si, int b, T (&l)[NU]) {
  static_assert(NU == 1 || NU == 2, "closed-form factor for NU <= 2");
  if constexpr (NU == 1) {
    l[0] = sqrt(Si[0]);
  } else {
    const T l00 = sqrt(Si[0]);
    const T l10 = Si[2] / l00;
    const T l11 = sqrt(fma(-l10, l10, Si[3]));
    l[0] = (b == 0) ? l00 : T(0);
    l[1] = (b == 0) ? l10 : l11;
  }
}

// The whole factor, for the row form, which applies L_k to every row at stage
// k: the lower Cholesky factor of the symmetric positive definite NU x NU
// matrix Si = S^-1 (NU <= 2); the entries above the diagonal are not set.  A
// non-positive pivot gives NaN or Inf; the Riccati pass has flagged that
// instance NOT_CONVEX already.  s00 is S[0][0] itself: at NU = 1 the factor is
// S^{-1/2}, taken straight from S by a reciprocal square root, so that its
// chain runs beside the chain of the reciprocal (S^-1 -> K -> P) and not
// behind it, with a third of the instructions of sqrt(1 / S).
__device__ __forceinline__ float rsq(float x) { return rsqrtf(x); }
__device__ __forceinline__ double rsq(double x) { return rsqrt(x); }

template <typename T, int NU>
__device__ __forceinline__ void chol_lower(T s00, const T (&Si)[NU][NU], T (&l)[NU][NU]) {
  static_assert(NU == 1 || NU == 2, "closed-form factor for NU <= 2");
  if constexpr (NU == 1) {
    l[0][0] = rsq(s00);
  } else {
    l[0][0] = sqrt(Si[0][0]);
    l[1][0] = Si[1][0] / l[0][0];
    l[1][1] = sqrt(fma(-l[1][0], l[1][0], Si[1][1]));
  }
}

// M = -W~ W~' straight into the register blocks of Mat (QSym: lane (bi, bj) of
// a group holds rows bi*BS.., columns bj*BS..).  Wt is the group's tile, column
// c of W~ at Wt + c*ld with all Mat::NV rows written (rows >= n are 0), so the
// BS values a lane needs per c are contiguous and entries with i >= n or
// j >= n come out 0.  Entries (i, j) and (j, i) accumulate the same products
// in the same order: the result is bitwise symmetric, which Mat::column()
// relies on (one published tile serves the row and the column vector).
template <typename T, class Mat>
__device__ __forceinline__ void neg_gram(Mat& M, const T* Wt, int ld, int n) {
  constexpr int BS = Mat::RPL;
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int c = 0; c < BS; ++c) M.m[r][c] = T(0);
  const T* wr = Wt + M.bi * BS;
  const T* wc = Wt + M.bj * BS;
#pragma unroll 4
  for (int k = 0; k < n; ++k) {
    T vr[BS], vc[BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      vr[r] = wr[k * ld + r];
      vc[r] = wc[k * ld + r];
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int c = 0; c < BS; ++c) M.m[r][c] = fma(-vr[r], vc[c], M.m[r][c]);
  }
}

}  // namespace mpcqp
