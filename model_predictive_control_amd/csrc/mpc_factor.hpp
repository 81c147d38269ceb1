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
