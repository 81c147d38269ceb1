// sweep_ieee.hpp -- the Goodnight sweep of the adjoint kernels (box_vjp.hip,
// loop_box_vjp.hip): QSym::sweep_col with an IEEE pivot reciprocal.  Both files
// are built without the approximate-division flags, so the two kernels sweep
// with the same instructions and a one-step episode of the loop adjoint equals
// the stand-alone adjoint bit for bit.
#pragma once
#include "quad.hpp"

namespace mpcqp {

// QSym::sweep_col (sigma = +1) with the pivot's reciprocal from an IEEE
// division instead of fast_rcp: a group sweeps |F| rows once, so the division
// is not on a long serial chain here.  Same selects as the layout's own sweep:
// row and column k are set, not produced by cancellation.
template <typename T, int BS>
__device__ __forceinline__ void sweep_col_ieee(QSym<T, BS>& M, int k, T d, const T (&colr)[BS],
                                               const T (&colc)[BS]) {
  const T rd = T(1) / d;
  T a[BS], srow[BS];
  bool ik[BS], jk[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    a[r] = colr[r] * rd;
    ik[r] = (M.bi * BS + r == k);
  }
#pragma unroll
  for (int c = 0; c < BS; ++c) {
    jk[c] = (M.bj * BS + c == k);
    srow[c] = jk[c] ? -rd : colc[c] * rd;
  }
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      const T gen = fma(-a[r], colc[c], M.m[r][c]);
      M.m[r][c] = ik[r] ? srow[c] : (jk[c] ? a[r] : gen);
    }
}

}  // namespace mpcqp
