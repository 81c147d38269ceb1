// dual_range_core.hpp -- what the two kernels of the dual range active set
// share: dual_range_kernel (solve_poly.hip) and poly_loop_kernel
// (loop_poly.hip), Goldfarb-Idnani in the row space on W = SWEEP_A(M) held in
// a Sym2D register grid (sym2d.hpp).
//
// Here: the dependence tolerance, the host-side defaults and the epilogue.
// The method's body (scan, ratio test, partial step, refresh) is still written
// out in each kernel, three times in all: dual_range_kernel, and the hard and
// the soft trip of poly_loop_kernel.  Moving it into functions here was tried
// and not kept, because poly_loop_kernel's register allocation does not
// survive it: see DESIGN.md 3.16, "One method, two kernels".  Known difference
// between the copies: the "ray" rule for dependent rows exists only in the
// soft trip.
#pragma once
#include "sym2d.hpp"

namespace mpcqp {

// W_pp at or below dep_tol M_pp: row p depends on the active rows
template <typename T>
constexpr T kDualDepTol = sizeof(T) == 8 ? T(1e-10) : T(1e-5);

// host side: the defaults behind max_iter <= 0 and tol <= 0
inline int dual_max_iter(int max_iter, int mt) { return max_iter > 0 ? max_iter : 4 * mt + 40; }
template <typename T>
inline T dual_tol(double tol) {
  return tol > 0 ? (T)tol : (sizeof(T) == 8 ? (T)1e-12 : (T)1e-6);
}

// z_j = z0 + Kt[:, j]' x - sum over the rows with y != 0 of Ut[r][j] y_r.  One
// function for the loop's plan (global Ut, Kt) and for its applied input
// (their LDS copies), so that u_t equals z_t[0..nu) bit for bit.
// z0: the state-independent part of the plan (-Hinv g_t)_j, 0 without one.
// (dual_range_kernel sums Kt' x, then -Hinv f1, then -Ut' y in a loop of its
// own: with f1 given the order differs, and so would the bits.)
template <typename T>
__device__ __forceinline__ T poly_epilogue(const T* Kt, const T* Ut, int64_t ld, int j, int nx,
                                           const T* x, T yi, uint64_t yact, T z0 = T(0)) {
  T acc = z0;
  for (int k = 0; k < nx; ++k) acc = fma(Kt[(int64_t)k * ld + j], x[k], acc);
  for (uint64_t mk = yact; mk; mk &= mk - 1) {
    const int r = uniform(__builtin_ctzll(mk));
    acc = fma(-Ut[(int64_t)r * ld + j], readlane(yi, r), acc);
  }
  return acc;
}

}  // namespace mpcqp
