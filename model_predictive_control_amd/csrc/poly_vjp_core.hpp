// poly_vjp_core.hpp -- what the polytope-QP adjoint kernels (poly_vjp.hip,
// loop_poly_vjp.hip) execute per step, on the Sym2D grid of
// dual_range_core.hpp, and what their entry points share on the host: the
// step from "M is in W" to the row variable e, the three accumulation tails
// (gf, Kt gz, -L'e), the scratch layout, the size checks and the shared-factor
// pointers.  A step of the loop adjoint equals the stand-alone adjoint bit for
// bit because both call this code, and both files are built with the forward's
// approximate-division flags (the pivot reciprocal is its fast_rcp).
//
// The algebra.  At the optimum the forward wrote the signed multipliers y with
// an exact 0 on every inactive row: A = {i : y_i != 0}.  With gz = dL/dz,
// gy = dL/dy and the shared factors of mpcqp_poly_setup (Hinv, Ut = C Hinv,
// M = C Hinv C', Kt = (-Hinv F)', L = -Ut F):
//     q   = Hinv gz,  r = Ut gz
//     e_A = M_AA^{-1} (r_A - gy_A),  e = 0 elsewhere
//     gf  = -(q - Ut_A' e_A),   gx0 = Kt gz - L_A' e_A
// The forward's refresh() has v = W w, y_A = -v_A for w_A = s0_A - b_A, and
// y_A = M_AA^{-1} (s0_A - b_A), so W_AA = -M_AA^{-1} for W = SWEEP_A(M):
// e_A = -(W w)_A with w_A = r_A - gy_A, 0 elsewhere -- |A| sweeps and one
// mat-vec, no iterations.
#pragma once
#include "dual_range_core.hpp"
#include "poly_ws.hpp"

namespace mpcqp {

// Sum over the wave in a fixed order; every lane receives the total.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  v += lane_step<1>(v);
  v += lane_step<2>(v);
  v += lane_step<4>(v);
  v += lane_step<8>(v);
  v += lane_step<16>(v);
  v += lane_step<32>(v);
  return v;
}

// One adjoint step of the wave's instance, with M in W as load_packed left it.
// (The load, and whether the step runs at all, stay with the callers: only
// poly_vjp_kernel reports a NaN/Inf in M, and with the load in here its
// <double, 5> takes 130 VGPRs instead of 128 and loses a wave of occupancy.)
// One row per lane: md = M_ii, act = "row i is in A" (y_i != 0; false off the
// rows, and on every lane of an instance that already failed), wi = r_i - gy_i.
//   W     <- SWEEP_A(M), the rows of A in ascending order at one sweep site.
//            A pivot at or below kDualDepTol M_kk (the forward's dependence
//            test) means the rows marked active are dependent: ok = false.
//   emask = A if ok, else 0
// Returns e_i, an exact zero off A and when a pivot failed.
template <typename T, int BS>
__device__ __forceinline__ T poly_vjp_step(Sym2D<T, BS>& W, T* buf, T* part, T md, bool act, T wi,
                                           bool& ok, uint64_t& emask) {
  const uint64_t amask = __builtin_amdgcn_ballot_w64(act);
  constexpr T dep_tol = kDualDepTol<T>;
  ok = true;
  for (uint64_t mk = amask; mk; mk &= mk - 1) {
    const int k = uniform(__builtin_ctzll(mk));
    T c[BS], cc[BS];
    const T d = W.column(k, buf, c, cc);
    if (!(d > dep_tol * fmax(readlane(md, k), T(1e-300)))) {
      ok = false;
      break;
    }
    W.sweep_col(k, T(1), d, c, cc);
  }
  const T v = matvec_lane_lds<T, BS>(W, act ? wi : T(0), buf, part);
  emask = ok ? amask : 0;
  return (ok && act) ? -v : T(0);
}

// gf_j = acc + sum over emask of Ut[r][j] e_r, rows in ascending order; acc is
// the caller's -q_j.
template <typename T>
__device__ __forceinline__ T gf_tail(const T* Ut, int nz, int j, T ei, uint64_t emask, T acc) {
  for (uint64_t mk = emask; mk; mk &= mk - 1) {
    const int r = uniform(__builtin_ctzll(mk));
    acc = fma(Ut[(int64_t)r * nz + j], readlane(ei, r), acc);
  }
  return acc;
}

// Kt gz (gz: the instance's n entries, null = 0): lane sums over j = lane,
// lane + 64, ..., one wave sum per k; lane k keeps entry k, the others 0.
template <typename T>
__device__ __forceinline__ T kt_gz(const T* Kt, const T* gz, int nz, int nx, int lane) {
  T gk = T(0);
  for (int k = 0; k < nx; ++k) {
    T s = T(0);
    for (int j = lane; j < nz; j += kWave)
      s = fma(Kt[(int64_t)k * nz + j], gz ? gz[j] : T(0), s);
    s = wave_sum(s);
    gk = (lane == k) ? s : gk;
  }
  return gk;
}

// acc - sum over emask of Lt[r][k] e_r, rows in ascending order, from a
// row-major table of `ld` columns (global L, or an LDS copy).
template <typename T>
__device__ __forceinline__ T lt_e_tail(const T* Lt, int ld, int k, T ei, uint64_t emask, T acc) {
  for (uint64_t mk = emask; mk; mk &= mk - 1) {
    const int r = uniform(__builtin_ctzll(mk));
    acc = fma(-Lt[r * ld + k], readlane(ei, r), acc);
  }
  return acc;
}

// ---------------------------------------------------------------- host side
// Scratch of both adjoints: -Hinv gz, then -Ut gz, `rows` rows each (batch, or
// steps x batch).
struct PolyVjpWs {
  int64_t oQ, oR, total;
};
static inline PolyVjpWs poly_vjp_ws(size_t es, int64_t rows, int n, int mt) {
  PolyVjpWs w;
  w.oQ = 0;
  w.oR = align256(rows * n * (int64_t)es);
  w.total = align256(w.oR + rows * mt * (int64_t)es);
  return w;
}

// What both entry points require of dtype, n, m and m_total = m + (nbox ? n : 0).
static inline bool poly_vjp_sizes_ok(int dtype, int n, int m, int mt) {
  return (dtype == MPCQP_F64 || dtype == MPCQP_F32) && n >= 1 && m >= 0 && mt >= 1 && mt <= 64;
}

// The shared factors of mpcqp_poly_setup in its workspace.
template <typename T>
struct PolyFactors {
  const T* M;                  // packed lower mt x mt
  const T* Hinv;               // n x n
  const T* Ut;                 // mt x n
  const T* Kt;                 // nx x n
  const T* L;                  // mt x nx
  const int32_t* flag;         // set by the shared inverse when H is not PD
};
template <typename T>
static inline void set_poly_factors(PolyFactors<T>& f, const void* workspace, const PolyWs& L) {
  const char* base = (const char*)workspace;
  f.M = (const T*)(base + L.oM); f.Hinv = (const T*)(base + L.oHinv);
  f.Ut = (const T*)(base + L.oUt); f.Kt = (const T*)(base + L.oKt);
  f.L = (const T*)(base + L.oL); f.flag = (const int32_t*)(base + L.oFlag);
}

}  // namespace mpcqp
