// loop_box.hip -- mpcqp_mpc_box_loop: the receding-horizon loop of an
// input-box MPC on a linear plant, T steps in ONE launch, four instances per
// wavefront (quad.hpp layout, one per 16-lane DPP row).
//
// Reference: the closed loop of session_1 (LinearSystem.simulate under a
// policy, LinearSystem.py:20-26; FHC.py:20-29) with the box-constrained MPC
// step of session_4 (MPCController.solve, main.py:115-116, input box
// main.py:68-69) as the policy, and simulate(x0, dynamics, n, policy)
// (main.py:270-271) as the loop.  Per step t and instance b:
//   f_t = F x_t                          (the condensed gradient; H, F of the
//                                          instance's LTI plant, mpcqp_condense)
//   z_t = argmin 1/2 z'Hz + f_t'z, lb <= z <= ub
//   x_{t+1} = A x_t + B u_0(z_t)
//
// Everything of an instance stays on chip for the whole episode: packed H and
// F in the group's LDS block, x_t in LDS, the active set in registers.  Each
// step is warm-started from the previous step's active set shifted one stage
// (row i takes the state of row i + nu; the last stage repeats): the matrix of
// the active set is H swept on its FREE rows only (H swept on F equals -H^-1
// swept back on the active rows), so a mostly saturated problem (config 2:
// ~80 % of the bounds active) starts from a handful of sweeps instead of n,
// and the Goldfarb-Idnani iterations only correct the guess (gi_box_st).  No
// Riccati, no -H^-1, no HBM traffic per step but x, u, the status and the
// (optional) input plan.
//
// mpcqp_mpc_box_loop_affine is the AFFINE instantiation: a per-step linear term
// g_t in the gradient (f_t = F x_t + g_t: reference tracking, batched.
// tracking_terms) and a plant disturbance w_t (x_{t+1} = A x_t + B u_0 + w_t),
// both read from HBM by the lane that owns the row (rows q and q + 16 of f,
// row q of x) one step ahead: g_{t+1} is loaded as soon as step t's f is in
// LDS and first used at the top of step t + 1, w_{t+1} as soon as w_t has gone
// into x_{t+1} and first used at the end of step t + 1, so their latency lies
// under the active set and each value needs one register, the one its
// predecessor has just left.  MPCQP_LOOP_COLD (a runtime argument of the same
// instantiation) starts every step from the empty set.
#include <type_traits>

#include "box_vjp_core.hpp"
#include "gi_box_core.hpp"
#include "quad_api.hpp"

namespace mpcqp {

template <typename T>
struct LoopArgs {
  int batch, nx, nu, N, n, steps;
  const T* H; int64_t sH;      // packed lower n(n+1)/2 per instance
  const T* F; int64_t sF;      // n x nx per instance (f = F x)
  const T* A; int64_t sA;      // plant nx x nx
  const T* B; int64_t sB;      // plant nx x nu
  const T* x0; int64_t sX0;
  const T* lb; int64_t slb;
  const T* ub; int64_t sub;
  T* xs;                       // (steps + 1) x batch x nx
  T* us;                       // steps x batch x nu
  T* zs;                       // optional steps x batch x n: the input plans
  int32_t* status;             // steps x batch
  int max_iter;
  T tol;
};

// The AFFINE instantiation's arguments: g_t of instance b at g + t * gT + b * sG
// (sG = 0, gT = n: shared by the batch; sG = n, gT = batch * n: per instance),
// w_t at w + (t * batch + b) * nx; either may be null.
template <typename T>
struct LoopAffineArgs : LoopArgs<T> {
  const T* g; int64_t sG, gT;
  const T* w;
  int cold;
};

template <typename T, bool AFFINE>
using LoopArgsOf = std::conditional_t<AFFINE, LoopAffineArgs<T>, LoopArgs<T>>;

template <typename T, int NX, int NU, int BS>
struct LoopLds {
  using Box = BoxLds<QSym<T, BS>>;
  static constexpr int NMAX = 4 * BS;
  static constexpr int PMAX = NMAX * (NMAX + 1) / 2;
  static constexpr int oP = Box::oEnd;          // packed H
  static constexpr int oF = oP + PMAX;          // F, NMAX x NX
  static constexpr int oA = oF + NMAX * NX;     // A, NX x NX
  static constexpr int oB = oA + NX * NX;       // B, NX x NU
  static constexpr int oX = oB + NX * NU;       // x_t
  static constexpr int oU = oX + NX;            // u_0
  static constexpr int oS = oU + NU;            // active-set flags (as T) for the shift
  static constexpr int size = oS + NMAX;
};

// Waves per SIMD the registers must allow.  A batch of 4096 is 1024 waves,
// one per SIMD: above BS = 2 the loop takes the whole register file (at 2
// waves per SIMD it spilled 176 B per lane at BS = 5).
template <typename T, int BS>
struct LoopOcc {
  static constexpr int w = BS <= 2 ? 4 : 1;
};

// Keyed reductions (Key, gi_box_core.hpp) per instantiation.  The affine fp64 NX = 4
// NU = 2 BS = 5 kernel sits at 256 VGPRs and would take one AGPR more (257: the
// bound of its registers 2 -> 1 waves): it keeps the compare-and-select
// reductions.
template <typename T, int NX, int NU, int BS, bool AFFINE>
struct LoopKeyed {
  static constexpr bool v = !(sizeof(T) == 8 && NX == 4 && NU == 2 && BS == 5 && AFFINE);
};

// The full-step trip, the ratio filter and the bound read-ahead (RowOwn's TRIP,
// gi_box_core.hpp) per instantiation; they exist on keyed rows only.
// The fp64 BS = 2 kernels would spill under the 128 VGPRs of their four-wave
// bound (120..124 VGPRs and no scratch -> 128 and 52..68 bytes per lane): they
// keep the general trip alone.  No other kernel gains scratch or loses a wave
// of its bound; fp64 BS = 5 (the config-2 loop) takes 13..23 AGPRs under its
// one-wave bound (252 -> 273 + 17).
template <typename T, int NX, int NU, int BS, bool AFFINE>
struct LoopTrip {
  static constexpr bool v = BS != 2;
};

// The masked sweep fix-up and the rates formed once per trip (RowOwn's LEAN,
// gi_box_core.hpp) per instantiation.  The five fp64 BS = 5 kernels could take
// them (269..279 + 13..23 -> 274..282 + 18..26 VGPRs + AGPRs, no scratch, one-wave
// bound), but the config-2 loop line did not move with them (190.3 M, 190.3 -
// 190.6, -> 190.9 M, 190.4 - 191.1 steps/s, ranges overlapping): no loop kernel
// takes them, and all compile to the streams they had before.
template <typename T, int NX, int NU, int BS, bool AFFINE>
struct LoopLean {
  static constexpr bool v = false;
};

// A wave-uniform pointer to global memory, held in scalar registers.
template <typename T>
using GlobalPtr = const __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ GlobalPtr<T> sbase(const T* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffull));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (GlobalPtr<T>)(((unsigned long long)hi << 32) | lo);
}

// The element `bytes` (a 32-bit per-lane offset) behind a scalar base: the
// address form global loads take without a per-lane 64-bit pointer.
template <typename T>
__device__ __forceinline__ T at_bytes(GlobalPtr<T> base, unsigned bytes) {
  return *(GlobalPtr<T>)((const __attribute__((address_space(1))) char*)base + bytes);
}

// The same address form for a store: base[row + off] with a wave-uniform row
// (64-bit, scalar) and a small per-lane off, formed at the store.
template <typename T>
__device__ __forceinline__ void put_at(T* base, int64_t row, unsigned off, T v) {
  const unsigned long long p = (unsigned long long)(base + row);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(p & 0xffffffffull));
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(p >> 32));
  asm volatile("" : "+v"(off));
  *(__attribute__((address_space(1))) T*)((__attribute__((address_space(1))) char*)(
        ((unsigned long long)hi << 32) | lo) + off * (unsigned)sizeof(T)) = v;
}

template <typename T, int NX, int NU, int BS, bool AFFINE = false>
__global__ __launch_bounds__(64, (LoopOcc<T, BS>::w)) void box_loop_kernel(
    LoopArgsOf<T, AFFINE> a) {
  using Lq = LoopLds<T, NX, NU, BS>;
  using Box = BoxLds<QSym<T, BS>>;
  constexpr int NMAX = Lq::NMAX;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
  const int b = blockIdx.x * 4 + g;
  [[maybe_unused]] const int64_t b0 = (int64_t)blockIdx.x * 4;  // the wave's first instance
  const bool live = b < a.batch;
  const int bl = live ? b : 0;
  const int n = a.n, nx = a.nx, nu = a.nu, P = n * (n + 1) / 2;
  T* gs = reinterpret_cast<T*>(smem_raw) + g * Lq::size;
  T* gb = gs + Box::oBuf;
  T* fs = gs + Box::oF;
  T* lbs = gs + Box::oLb;
  T* ubs = gs + Box::oUb;
  T* Ps = gs + Lq::oP;
  T* Fs = gs + Lq::oF;
  T* As = gs + Lq::oA;
  T* Bs = gs + Lq::oB;
  T* xg = gs + Lq::oX;
  T* ug = gs + Lq::oU;
  T* sg = gs + Lq::oS;

  // ------------------------------------------------------------- stage in
  {
    const T* Hb = a.H + (int64_t)bl * a.sH;
    for (int e = q; e < Lq::PMAX; e += 16) Ps[e] = e < P ? Hb[e] : T(0);
    const T* Fb = a.F + (int64_t)bl * a.sF;
    for (int e = q; e < NMAX * NX; e += 16) {
      const int i = e / NX, j = e - i * NX;
      Fs[e] = (i < n && j < nx) ? Fb[i * nx + j] : T(0);
    }
    for (int e = q; e < NX * NX; e += 16) {
      const int i = e / NX, j = e - i * NX;
      As[e] = (i < nx && j < nx) ? a.A[(int64_t)bl * a.sA + i * nx + j] : T(0);
    }
    for (int e = q; e < NX * NU; e += 16) {
      const int i = e / NU, j = e - i * NU;
      Bs[e] = (i < nx && j < nu) ? a.B[(int64_t)bl * a.sB + i * nu + j] : T(0);
    }
    if (q < NX) xg[q] = q < nx ? a.x0[(int64_t)bl * a.sX0 + q] : T(0);
  }
  bool nonfinite = false, badbox = false;
  for (int i = q; i < NMAX; i += 16) {
    const bool v = live && i < n;
    const T li = (v && a.lb) ? a.lb[(int64_t)b * a.slb + i] : -Lim<T>::inf();
    const T ui = (v && a.ub) ? a.ub[(int64_t)b * a.sub + i] : Lim<T>::inf();
    lbs[i] = li;
    ubs[i] = ui;
    badbox |= v && (!(li <= ui) || li == Lim<T>::inf() || ui == -Lim<T>::inf());
  }
  __syncthreads();
  for (int e = q; e < P; e += 16) nonfinite |= live && !finite(Ps[e]);
  for (int e = q; e < NMAX * NX; e += 16) nonfinite |= live && !finite(Fs[e]);
  const unsigned long long gmask = 0xFFFFull << (16 * g);
  const int code0 = ((__ballot(nonfinite) & gmask) != 0)
                        ? MPCQP_STATUS_NONFINITE
                        : (((__ballot(badbox) & gmask) != 0) ? MPCQP_STATUS_INFEASIBLE
                                                              : MPCQP_STATUS_OPTIMAL);

#ifdef MPCQP_PHASE_TIMING
  PhaseClock mpcqp_clk;
#endif
  QSym<T, BS> M;
  M.init(lane);
  int st[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) st[r] = (M.bi * BS + r < n) ? 0 : 3;  // cold first step
  int failed = MPCQP_STATUS_OPTIMAL;  // code of the group's first failed step
  // The states this lane's rows may take from the shift: bit 0 = the lower
  // bound is finite (state 1), bit 1 = the upper one (state 2).  The bounds may
  // differ along the horizon, and a row put on an infinite bound makes z
  // infinite (two such rows: NaN multipliers that the release phase cannot
  // order).
  int okst[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    const int i = M.bi * BS + r;
    okst[r] = (lbs[i] > -Lim<T>::inf() ? 1 : 0) | (ubs[i] < Lim<T>::inf() ? 2 : 0);
  }

  // AFFINE: this lane's entries of g (rows q and, where NMAX > 16, q + 16 of f)
  // and of w (row q of x), loaded one step ahead into the register that the
  // step before has just left; 0 where there is none.  Where four waves share
  // a SIMD (BS <= 2: n <= 8, 128 VGPRs) lanes 8.. of the group have no row of
  // g, and w_t[j] travels in lane 8 + j of g's register (WPACK): the loads are
  // per lane, so the two halves of the register are reloaded at different
  // points of the step.  The address is a wave-uniform base of the step (in
  // scalar registers: sbase) plus a small per-lane offset, so that no per-lane
  // pointer lives across the step.
  constexpr bool WPACK = BS <= 2;
  [[maybe_unused]] T gn0 = T(0), gn1 = T(0), wn = T(0);
  [[maybe_unused]] auto fetch_g = [&](int t) {
    if constexpr (AFFINE) {
      if (live && a.g) {
        const auto gt = sbase(a.g + (int64_t)t * a.gT + b0 * a.sG);
        unsigned o = a.sG ? (unsigned)(g * n + q) : (unsigned)q;
        asm volatile("" : "+v"(o));  // formed here, every step: nothing of it kept in the loop
        if (q < n) gn0 = at_bytes(gt, o * (unsigned)sizeof(T));
        if constexpr (NMAX > 16)
          if (q + 16 < n) gn1 = at_bytes(gt, (o + 16u) * (unsigned)sizeof(T));
      }
    }
  };
  [[maybe_unused]] auto fetch_w = [&](int t) {
    if constexpr (AFFINE) {
      const int j = WPACK ? q - 8 : q;
      if (live && a.w && j >= 0 && j < nx) {
        const auto wt = sbase(a.w + ((int64_t)t * a.batch + b0) * nx);
        unsigned o = (unsigned)(g * nx + j);
        asm volatile("" : "+v"(o));
        (WPACK ? gn0 : wn) = at_bytes(wt, o * (unsigned)sizeof(T));
      }
    }
  };
  if constexpr (AFFINE)
    if (a.steps > 0) {
      fetch_g(0);
      fetch_w(0);
    }

  for (int t = 0; t < a.steps; ++t) {
    // record x_t; f = F x_t (rows q, q + 16 of the group)
    if constexpr (AFFINE) {  // (the stores by put_at: no per-lane pointers kept in the loop)
      if (live && q < nx) put_at(a.xs, ((int64_t)t * a.batch + b0) * nx, (unsigned)(g * nx + q), xg[q]);
    } else {
      if (live && q < nx) a.xs[((int64_t)t * a.batch + b) * nx + q] = xg[q];
    }
    // A NaN/Inf in x_t (from x0, A, B or a failed step; H and F are checked at
    // stage-in) makes f non-finite: every violation is then NaN, the group
    // "settles" and the final clamp turns the NaN z into a bound.  Every lane
    // of the group reads the same x_t, so the flag needs no ballot.
    bool nfx = false;
#pragma unroll
    for (int j = 0; j < NX; ++j) nfx |= !finite(xg[j]);
    if constexpr (AFFINE) {
#ifdef MPCQP_BOX_LOOP_PLAIN_LOAD  // A/B variant: load g_t where it is used
      if (t > 0) fetch_g(t);
#endif
      // a non-finite g_t fails this group alone (its own ballot bits)
      nfx |= (__ballot((!finite(gn0) && !(WPACK && q >= 8)) || !finite(gn1)) & gmask) != 0;
    }
    for (int i = q; i < NMAX; i += 16) {
      T s = T(0);
#pragma unroll
      for (int j = 0; j < NX; ++j) s = fma(Fs[i * NX + j], xg[j], s);
      if constexpr (AFFINE) s += i < 16 ? gn0 : gn1;
      fs[i] = s;
    }
    lds_exchange();
#ifndef MPCQP_BOX_LOOP_PLAIN_LOAD
    // g_{t+1}: in flight during the active set below; never past the last row
    if constexpr (AFFINE)
      if (t + 1 < a.steps) fetch_g(t + 1);
#endif
    bool nf = false;
    M.load_packed(Ps, n, nf);
    // sweep H on the free rows of the warm-start set (box_vjp_core.hpp)
    const unsigned fmask = free_row_mask(M, st, g);
    // NONFINITE goes before INFEASIBLE (code0 holds either), as in box_quad_kernel;
    // the step then skips gi_box_st, writes NaN and leaves the next one cold.
    // A failed step makes x NaN for the rest of the episode, whose steps
    // repeat the code of that first failure (its cause), not NONFINITE.
    int code = nfx ? MPCQP_STATUS_NONFINITE : code0;
    if (failed != MPCQP_STATUS_OPTIMAL) code = failed;
    const int sweeps = __popc(fmask);
    const bool okp = sweep_free_rows(M, gb, fmask, [&](int k, T d, const T(&colr)[BS],
                                                       const T(&colc)[BS]) {
      M.sweep_col(k, T(1), d, colr, colc);
    });
    if (code == MPCQP_STATUS_OPTIMAL && !okp) code = MPCQP_STATUS_NOT_CONVEX;
    T zr[BS];
    int iters = 0;
    using Own = RowOwn<QSym<T, BS>, QRowOwned<QSym<T, BS>>::v, LoopKeyed<T, NX, NU, BS, AFFINE>::v,
                       LoopTrip<T, NX, NU, BS, AFFINE>::v, LoopLean<T, NX, NU, BS, AFFINE>::v>;
    const int c2 = gi_box_st<true, Own>(M, gb, fs, lbs, ubs, n, a.max_iter, a.tol,
                                        live && code == MPCQP_STATUS_OPTIMAL, zr, iters,
                                        st MPCQP_CLK_ARG);
    if (code == MPCQP_STATUS_OPTIMAL) code = c2;
    const bool okc = code == MPCQP_STATUS_OPTIMAL || code == MPCQP_STATUS_MAXITER;
    if (!okc) {
      failed = code;
#pragma unroll
      for (int r = 0; r < BS; ++r) zr[r] = __builtin_nan("");
    }
    // outputs of the step; u_0 and the active set through LDS
    if (M.bj == 0) {
#pragma unroll
      for (int r = 0; r < BS; ++r) {
        const int i = M.bi * BS + r;
        if (i < NU) ug[i] = zr[r];
        if (i < NMAX) sg[i] = (T)st[r];
        if constexpr (AFFINE) {
          if (live && a.zs && i < n)
            put_at(a.zs, ((int64_t)t * a.batch + b0) * n, (unsigned)(g * n + i), zr[r]);
        } else {
          if (live && a.zs && i < n) a.zs[((int64_t)t * a.batch + b) * n + i] = zr[r];
        }
      }
    }
    const int word = (code & 0xff) | (((iters + sweeps) & 0xffff) << 8);
    if constexpr (AFFINE) {
      if (live && q == 0) put_at(a.status, (int64_t)t * a.batch + b0, (unsigned)g, (int32_t)word);
    } else {
      if (live && q == 0) a.status[(int64_t)t * a.batch + b] = word;
    }
    lds_exchange();
    if constexpr (AFFINE) {
      if (live && q < nu) put_at(a.us, ((int64_t)t * a.batch + b0) * nu, (unsigned)(g * nu + q), ug[q]);
    } else {
      if (live && q < nu) a.us[((int64_t)t * a.batch + b) * nu + q] = ug[q];
    }
    // plant: x_{t+1} = A x_t + B u_0
    T xn = T(0);
    if (q < NX) {
#pragma unroll
      for (int j = 0; j < NX; ++j) xn = fma(As[q * NX + j], xg[j], xn);
#pragma unroll
      for (int j = 0; j < NU; ++j) xn = fma(Bs[q * NU + j], ug[j], xn);
    }
#ifdef MPCQP_BOX_LOOP_PLAIN_LOAD
    if constexpr (AFFINE)
      if (t > 0) fetch_w(t);
#endif
    if constexpr (AFFINE) xn += WPACK ? dpp<0x128>(gn0) : wn;  // row_ror:8 = lane ^ 8
#ifndef MPCQP_BOX_LOOP_PLAIN_LOAD
    // w_{t+1}, first used a whole step from here
    if constexpr (AFFINE)
      if (t + 1 < a.steps) fetch_w(t + 1);
#endif
    // warm start of the next step: row i takes row i + nu's state (the last
    // stage keeps its own); a failed step restarts cold
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      const int i = M.bi * BS + r;
      const int src = i + nu < n ? i + nu : i;
      const int s = okc ? ((int)sg[src] & okst[r]) : 0;  // states are 0, 1, 2
      if constexpr (AFFINE)
        st[r] = i < n && !a.cold ? s : (i < n ? 0 : 3);
      else
        st[r] = i < n ? s : 3;
    }
    lds_exchange();
    if (q < NX) xg[q] = xn;
    lds_exchange();
  }
  if constexpr (AFFINE) {
    if (live && q < nx)
      put_at(a.xs, ((int64_t)a.steps * a.batch + b0) * nx, (unsigned)(g * nx + q), xg[q]);
  } else {
    if (live && q < nx) a.xs[((int64_t)a.steps * a.batch + b) * nx + q] = xg[q];
  }
}

template <typename T, int NX, int NU, int BS, bool AFFINE>
static int launch_loop(const LoopArgsOf<T, AFFINE>& a, hipStream_t st) {
  using Lq = LoopLds<T, NX, NU, BS>;
  const size_t bytes = (size_t)4 * Lq::size * sizeof(T);
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)box_loop_kernel<T, NX, NU, BS, AFFINE>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(box_loop)");
  }
  hipLaunchKernelGGL((box_loop_kernel<T, NX, NU, BS, AFFINE>),
                     dim3((unsigned)((a.batch + 3) / 4)), dim3(64), bytes, st, a);
  MPCQP_CHECK_LAUNCH("box_loop_kernel");
  return MPCQP_OK;
}

template <typename T, bool AFFINE>
static int loop_t(const LoopArgsOf<T, AFFINE>& a, hipStream_t st) {
  return dispatch_nxnu(a.nx, a.nu, [&](auto cx, auto cu) {
    return dispatch_bs<4>(a.n, [&](auto bs) {
      return launch_loop<T, decltype(cx)::value, decltype(cu)::value, decltype(bs)::value,
                         AFFINE>(a, st);
    });
  });
}

// Both entry points: g == w == nullptr and flags == 0 launch the kernels of
// mpcqp_mpc_box_loop.
static int box_loop_entry(const char* who, int dtype, int batch, int nx, int nu, int N, int steps,
                          int flags, const void* H, int64_t strideH, const void* F,
                          int64_t strideF, const void* A, int64_t strideA, const void* Bm,
                          int64_t strideB, const void* x0, int64_t strideX0, const void* lb,
                          int64_t strideLb, const void* ub, int64_t strideUb, const void* g,
                          int64_t strideG, const void* w, void* xs, void* us, void* zs,
                          int32_t* status, int max_iter, double tol, void* stream) {
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "%s: bad dtype %d", who, dtype);
  MPCQP_CHECK_ARG(batch >= 0 && N >= 1 && steps >= 0, "%s: bad sizes", who);
  MPCQP_CHECK_LOOP_SIZES(who, nx, nu, N);
  MPCQP_CHECK_ARG((flags & ~MPCQP_LOOP_COLD) == 0, "%s: unknown flags 0x%x", who, flags);
  MPCQP_CHECK_ARG(H && F && A && Bm && x0 && xs && (steps == 0 || (us && status)),
                  "%s: H, F, A, B, x0, xs (and us, status for steps > 0) are required", who);
  MPCQP_CHECK_ARG(strideH >= 0 && strideF >= 0 && strideA >= 0 && strideB >= 0 &&
                      strideX0 >= 0 && strideLb >= 0 && strideUb >= 0,
                  "%s: negative stride", who);
  MPCQP_CHECK_ARG(!g || strideG == 0 || strideG == N * nu,
                  "%s: strideG=%lld is neither 0 nor n=%d", who, (long long)strideG, N * nu);
  if (batch == 0) return MPCQP_OK;
  auto fill = [&](auto& a, auto tp) {
    using T = decltype(tp);
    a.batch = batch; a.nx = nx; a.nu = nu; a.N = N; a.n = N * nu; a.steps = steps;
    a.H = (const T*)H; a.sH = strideH; a.F = (const T*)F; a.sF = strideF;
    a.A = (const T*)A; a.sA = strideA; a.B = (const T*)Bm; a.sB = strideB;
    a.x0 = (const T*)x0; a.sX0 = strideX0;
    a.lb = (const T*)lb; a.slb = strideLb; a.ub = (const T*)ub; a.sub = strideUb;
    a.xs = (T*)xs; a.us = (T*)us; a.zs = (T*)zs; a.status = status;
    a.max_iter = max_iter > 0 ? max_iter : 3 * N * nu + 30;
    a.tol = tol > 0 ? (T)tol : (dtype == MPCQP_F64 ? (T)1e-12 : (T)1e-6);
  };
  auto run = [&](auto tp) {
    using T = decltype(tp);
    hipStream_t st = (hipStream_t)stream;
    if (g || w || flags) {
      LoopAffineArgs<T> a;
      fill(a, tp);
      a.g = (const T*)g; a.sG = strideG;
      a.gT = strideG == 0 ? (int64_t)N * nu : (int64_t)batch * N * nu;
      a.w = (const T*)w;
      a.cold = (flags & MPCQP_LOOP_COLD) ? 1 : 0;
      return loop_t<T, true>(a, st);
    }
    LoopArgs<T> a;
    fill(a, tp);
    return loop_t<T, false>(a, st);
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}

}  // namespace mpcqp

extern "C" int mpcqp_mpc_box_loop(int dtype, int batch, int nx, int nu, int N, int steps,
                                  const void* H, int64_t strideH, const void* F, int64_t strideF,
                                  const void* A, int64_t strideA, const void* Bm, int64_t strideB,
                                  const void* x0, int64_t strideX0, const void* lb,
                                  int64_t strideLb, const void* ub, int64_t strideUb, void* xs,
                                  void* us, void* zs, int32_t* status, int max_iter, double tol,
                                  void* stream) {
  return mpcqp::box_loop_entry("mpcqp_mpc_box_loop", dtype, batch, nx, nu, N, steps, 0, H, strideH,
                               F, strideF, A, strideA, Bm, strideB, x0, strideX0, lb, strideLb, ub,
                               strideUb, nullptr, 0, nullptr, xs, us, zs, status, max_iter, tol,
                               stream);
}

extern "C" int mpcqp_mpc_box_loop_affine(int dtype, int batch, int nx, int nu, int N, int steps,
                                         int flags, const void* H, int64_t strideH, const void* F,
                                         int64_t strideF, const void* A, int64_t strideA,
                                         const void* Bm, int64_t strideB, const void* x0,
                                         int64_t strideX0, const void* lb, int64_t strideLb,
                                         const void* ub, int64_t strideUb, const void* g,
                                         int64_t strideG, const void* w, void* xs, void* us,
                                         void* zs, int32_t* status, int max_iter, double tol,
                                         void* stream) {
  return mpcqp::box_loop_entry("mpcqp_mpc_box_loop_affine", dtype, batch, nx, nu, N, steps, flags,
                               H, strideH, F, strideF, A, strideA, Bm, strideB, x0, strideX0, lb,
                               strideLb, ub, strideUb, g, strideG, w, xs, us, zs, status, max_iter,
                               tol, stream);
}
