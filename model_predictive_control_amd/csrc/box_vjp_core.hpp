// box_vjp_core.hpp -- what the box-QP adjoint kernels (box_vjp.hip,
// loop_box_vjp.hip) execute per step, on the QSym layout of quad.hpp: the
// free-row mask of a group, the wave-uniform sweep loop over the free rows
// (also the warm-start pre-sweep of loop_box.hip), the IEEE sweep body, the
// step from "H is in M" to d and nu, and the fold of d z' onto the packed
// lower triangle.  A one-step episode of the loop adjoint equals the
// stand-alone adjoint bit for bit because both call this code, and both files
// are built without the approximate-division flags.
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

// The mask of group g's rows in state 0 (free): bit bi*BS + r from the bj == 0
// lane of row block bi.  Group-uniform.
template <typename T, int BS>
__device__ __forceinline__ unsigned free_row_mask(const QSym<T, BS>& M, const int (&st)[BS],
                                                  int g) {
  unsigned fmask = 0;
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    const unsigned long long bal = __ballot(M.bj == 0 && st[r] == 0);
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
      if ((bal >> (16 * g + 4 * bb)) & 1ull) fmask |= 1u << (bb * BS + r);
  }
  return fmask;
}

// M = SWEEP_F(M) on the rows of fmask, lowest first, in wave-uniform trips: the
// four groups of a wave hold different masks, so the loop runs while any group
// has a row left, every group passes every LDS publish of QSym::column, and a
// group with nothing left discards what it read.  sweep_col(k, d, colr, colc)
// is the sweep body on pivot k with its column fetched.  Returns "every pivot
// of this group was > 0".
template <typename T, int BS, class SweepCol>
__device__ __forceinline__ bool sweep_free_rows(QSym<T, BS>& M, T* gb, unsigned fmask,
                                                SweepCol&& sweep_col) {
  bool okp = true;
  while (__any(fmask != 0)) {
    const bool has = fmask != 0;
    const int k = has ? __builtin_ctz(fmask) : 0;
    fmask = has ? fmask & (fmask - 1) : 0u;
    T colr[BS], colc[BS];
    const T d = M.column(k, gb, colr, colc);
    if (has) {
      okp = okp && d > T(0);
      sweep_col(k, d, colr, colc);
    }
  }
  return okp;
}

// One adjoint step of group g with H already in M and the rows z, gz, lb, ub
// in the group's LDS; `run` says whether the instance is to run at all.
//   st   the rows' states (0 free, 1 at lb, 2 at ub, 3 past n), compared
//        exactly; lb == ub == z counts as "at lb"
//   M    <- SWEEP_F(H): M_FF = -H_FF^-1, M_AF = H_AF H_FF^-1
//   out  = M [gz_F; 0], so d_F = out_F and nu_A = gz_A - out_A
// zr, st, dr, nur are those of rows bi*BS + r of this lane; dr and nur are
// exact zeros unless the step is good.  Returns good = run and every pivot > 0
// (run && !good: H_FF is not positive definite).
template <typename T, int BS>
__device__ __forceinline__ bool box_vjp_step(QSym<T, BS>& M, T* gb, const T* zs, const T* gzs,
                                             const T* lbs, const T* ubs, int n, int g, bool run,
                                             T (&zr)[BS], int (&st)[BS], T (&dr)[BS],
                                             T (&nur)[BS]) {
  T gr[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    const int i = M.bi * BS + r;
    zr[r] = zs[i];
    gr[r] = gzs[i];
    st[r] = i < n ? (zr[r] == lbs[i] ? 1 : (zr[r] == ubs[i] ? 2 : 0)) : 3;
  }
  unsigned fmask = free_row_mask(M, st, g);  // (the ballots: by every lane of the wave)
  if (!run) fmask = 0;
  const bool okp = sweep_free_rows(M, gb, fmask, [&](int k, T d, const T(&colr)[BS],
                                                     const T(&colc)[BS]) {
    sweep_col_ieee(M, k, d, colr, colc);
  });
  const bool good = run && okp;
  T w[BS], out[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) w[r] = (good && st[r] == 0) ? gr[r] : T(0);
  M.matvec(w, gb, out);
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    dr[r] = (good && st[r] == 0) ? out[r] : T(0);
    nur[r] = (good && (st[r] == 1 || st[r] == 2)) ? gr[r] - out[r] : T(0);
  }
  return good;
}

// dL/dH (full, unsymmetrised) = d z', folded onto the packed lower triangle by
// the block owners on and below the diagonal: store(i(i+1)/2 + j, v) with
// v = d_i z_j + d_j z_i for j < i and d_i z_i for j == i.  ds and zs hold d and
// z of the group in LDS (for the column block), dr and zr this lane's rows.
template <typename T, int BS, class Store>
__device__ __forceinline__ void fold_dz(const QSym<T, BS>& M, const T* ds, const T* zs,
                                        const T (&dr)[BS], const T (&zr)[BS], int n,
                                        Store&& store) {
  if (M.bi >= M.bj) {
    T dc[BS], zc[BS];
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      dc[c] = ds[M.bj * BS + c];
      zc[c] = zs[M.bj * BS + c];
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        const int i = M.bi * BS + r, j = M.bj * BS + c;
        if (i < n && j <= i) {
          const T v = i == j ? dr[r] * zr[r] : fma(dr[r], zc[c], dc[c] * zr[r]);
          store(i * (i + 1) / 2 + j, v);
        }
      }
  }
}

}  // namespace mpcqp
