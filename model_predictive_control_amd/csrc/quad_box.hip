// quad_box.hip -- the box-QP kernels for n <= 32 with FOUR instances per
// wavefront (quad.hpp): one QP per 16-lane DPP row on a 4 x 4 grid of register
// blocks.  Two kernels:
//   box_quad_kernel  -- mpcqp_solve_box: packed H in, n sweeps form -H^{-1},
//                       then the group-wise Goldfarb-Idnani active set;
//   mpc_group_kernel -- mpcqp_mpc_box: per-instance plant in, same active set;
//                       nothing but (A, B, x0, bounds) and z cross HBM.
//
// mpc_group_kernel builds M = -H^{-1} from one backward Riccati pass
//     S_k = R + B_k'P_{k+1}B_k,  K_k = -S_k^{-1} B_k'P_{k+1}A_k,
//     P_k = Q + A_k'P_{k+1}A_k + A_k'P_{k+1}B_k K_k,   P_N = Qf
// without ever forming H:  H = T' diag(S_k) T with T: u -> (u_k - K_k x_k(u))
// unit lower block triangular, so H^{-1} = W diag(S_k^{-1}) W' with W = T^{-1}
// (mpc_factor.hpp).  In order:
//   1. stage in: every global load of the group is issued before the first wait;
//   2. Riccati stage N-1-t next to free-response (x-bar) stage t, one loop.
//      Row form (QMpcRows; nx <= 2): the same loop generates
//      W~ = W diag(chol(S_k^{-1})) by rows, backward in the column stage: at
//      Riccati step j, K_j, A_j + B_j K_j, B_j and S_j^-1 are in the registers
//      of every lane, and lane q, which owns rows q and q + 16, writes its
//      entries of the nu columns of stage j from one 1 x NX row vector per
//      row (mpc_factor.hpp) -- no LDS read at all.  f comes from the
//      x0-independent backward form of the adjoint, y_k = Pi_k xbar_k + pi_k:
//          Pi_k = Q + A_k' Pi_{k+1} A_k,  pi_k = A_k'(Pi_{k+1} c_k + pi_{k+1}),
//          f_k = (B_k' Pi_{k+1}) xbar_{k+1} + B_k' pi_{k+1},   Pi_N = Qf, pi_N = 0
//      (pi only with a drift), whose recursion also runs in this loop; the
//      row's lane catches g_k = B_k' Pi_{k+1} at backward step k and
//      xbar_{k+1} at forward step k, and f is one short dot product per row
//      after the loop;
//   3. two-loop form (the other instantiations): every lane rolls its
//      column(s) of W~ forward in lockstep over the stages in a second loop
//      (closed loop from u_j = L_j[:, b]; K_k and A_k + B_k K_k are broadcast
//      LDS reads), next to the backward adjoint y_k = Q xbar_k + A_k'y_{k+1}
//      that yields f_k = B_k'y_{k+1};
//   4. M = -W~ W~' accumulated from the LDS tile straight into the register
//      blocks, bitwise symmetric;
//   5. Goldfarb-Idnani on M (gi_box_core.hpp).
// (mpc_box.hip, the one-QP-per-wave path, builds the columns of H^{-1} one by
// one instead and serves as the independent comparator in the tests.)
#include "mpc_factor.hpp"
#include "gi_box_core.hpp"
#include "quad_api.hpp"

namespace mpcqp {

template <typename T, int BS>
struct QuadOcc {
  // fp64 BS = 5 (n = 17..20, BASELINE config 2) needs ~190 VGPRs
  static constexpr int w = sizeof(T) == 8 ? (BS <= 3 ? 4 : (BS == 4 ? 3 : (BS == 5 ? 2 : 1)))
                                           : (BS <= 3 ? 4 : (BS <= 5 ? 3 : 2));
};

template <typename T, int BS>
__global__ __launch_bounds__(64, (QuadOcc<T, BS>::w)) void box_quad_kernel(BoxArgsQ<T> a) {
#ifdef MPCQP_PHASE_TIMING
  PhaseClock mpcqp_clk;
#endif
  using L = BoxLds<QSym<T, BS>>;
  constexpr int NMAX = L::NMAX;
  constexpr int PMAX = NMAX * (NMAX + 1) / 2;
  constexpr int GSZ = L::oEnd + PMAX;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
  const int b = blockIdx.x * 4 + g;
  const bool live = b < a.batch;
  const int bl = live ? b : 0;
  const int n = a.n, P = n * (n + 1) / 2;
  T* gs = reinterpret_cast<T*>(smem_raw) + g * GSZ;
  T* gb = gs + L::oBuf;
  T* fs = gs + L::oF;
  T* lbs = gs + L::oLb;
  T* ubs = gs + L::oUb;
  T* Ps = gs + L::oEnd;
  {
    constexpr int MAXT = (PMAX + 15) / 16;
    const T* Hb = a.H + (int64_t)bl * a.sH;
    T tmp[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int e = q + 16 * t;
      tmp[t] = (e < P) ? Hb[e] : T(0);
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int e = q + 16 * t;
      if (e < P) Ps[e] = tmp[t];
    }
  }
  bool nonfinite = false, badbox = false;
  for (int i = q; i < NMAX; i += 16) {
    const bool v = live && i < n;
    const T fi = v ? a.f[(int64_t)b * a.sf + i] : T(0);
    const T li = (v && a.lb) ? a.lb[(int64_t)b * a.slb + i] : -Lim<T>::inf();
    const T ui = (v && a.ub) ? a.ub[(int64_t)b * a.sub + i] : Lim<T>::inf();
    fs[i] = fi;
    lbs[i] = li;
    ubs[i] = ui;
    nonfinite |= v && !finite(fi);
    badbox |= v && (!(li <= ui) || li == Lim<T>::inf() || ui == -Lim<T>::inf());
  }
  __syncthreads();
  QSym<T, BS> M;
  M.init(lane);
  M.load_packed(Ps, n, nonfinite);
  // group-wide flags (OR over the 16 lanes of the row)
  const unsigned long long gmask = 0xFFFFull << (16 * g);
  const bool g_nonfinite = (__ballot(nonfinite) & gmask) != 0;
  const bool g_badbox = (__ballot(badbox) & gmask) != 0;
  int code = MPCQP_STATUS_OPTIMAL;
  if (g_nonfinite) code = MPCQP_STATUS_NONFINITE;
  else if (g_badbox) code = MPCQP_STATUS_INFEASIBLE;
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const T d = M.sweep(k, T(1), gb);
    ok &= d > T(0);
  }
  if (code == MPCQP_STATUS_OPTIMAL && !ok) code = MPCQP_STATUS_NOT_CONVEX;
  T zr[BS];
  int iters = 0;
  const int c2 = gi_box(M, gb, fs, lbs, ubs, n, a.max_iter, a.tol,
                        live && code == MPCQP_STATUS_OPTIMAL, zr, iters MPCQP_CLK_ARG);
  if (code == MPCQP_STATUS_OPTIMAL) code = c2;
  if (code != MPCQP_STATUS_OPTIMAL && code != MPCQP_STATUS_MAXITER) {
#pragma unroll
    for (int r = 0; r < BS; ++r) zr[r] = __builtin_nan("");
  }
  if (live && M.bj == 0) {
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      const int i = M.bi * BS + r;
      if (i < n) a.z[(int64_t)b * n + i] = zr[r];
    }
  }
  if (live && q == 0) a.status[b] = (code & 0xff) | ((iters & 0xffff) << 8);
}

// ----------------------------------------------------------- fused kernel
// Which instantiations of mpc_group_kernel generate W~ by rows inside the
// Riccati loop (true) and which keep the two-loop setup, W~ by columns in a
// second loop (false).  The row form carries, next to the Riccati state, one
// NX-vector per owned row for each of Psi, g and x-bar plus the NX x NX
// Lyapunov matrix Pi.  Registers, scratch bytes per lane and occupancy bound
// of the built kernels (two-loop -> rows):
//   fp64 NX = 4:                 scratch 0..52 -> 364..528 bytes (BS <= 5)
//   fp32 NX = 4:                 124..167 -> 168..228 VGPRs, bound 3..4 -> 2..3 waves
//   fp64 NX = 2, NU = 2, BS <= 3: scratch 0..24 -> 72 bytes under the 128 VGPRs
//                                 of their four-wave bound, and measured 3-6 %
//                                 slower (B = 4096: n = 4 13.1 -> 13.6 us, n = 8
//                                 time-varying 18.0 -> 19.0, n = 12 30.4 -> 31.5)
// Those stay on two loops.  Every other one takes the row form: the config-2
// instantiation (fp64 NX = 2 NU = 1 BS = 5) has 209 VGPRs and no scratch both
// ways, none gains scratch, and only fp64 NX = 2 NU = 1 BS = 1 loses a wave of
// its occupancy bound (86 -> 115 VGPRs, 5 -> 4) while measuring faster (n = 1
// 6.1 -> 5.7 us, n = 4 11.4 -> 10.7).
template <typename T, int NX, int NU, int BS>
struct QMpcRows {
  static constexpr bool v = NX <= 2 && !(sizeof(T) == 8 && NU == 2 && BS <= 3);
};

// The row form's setup loop per combination of the wave-uniform launch flags
// (tv, drift), chosen in front of the loop, so that no stage tests them and
// the read-ahead of c is not carried without a drift (level 1), and with two
// stages per trip on top (level 2; mpc_setup_loop.inc, mpc_setup_stage.inc).
// -DMPCQP_SETUP_UNIFORM=0 builds the tree without either (tools/ab_build.sh),
// = 1 caps the level at 1.  The loops change the register allocation.  Built
// objects, VGPRs / scratch bytes per lane, parent -> level 1 / level 2:
//   fp64 NU = 1 BS = 1: 115 / 0 -> 128 / 20,  128 / 184   (bound 4 waves: 128 VGPRs)
//   fp64 NU = 1 BS = 2: 115 / 0 -> 128 / 20,  128 / 172
//   fp64 NU = 1 BS = 3: 126 / 0 -> 128 / 20,  128 / 164
//   fp64 NU = 1 BS = 4: 148 / 0 -> 148 / 0,   168 / 24    (bound 3 waves: 168 VGPRs)
//   fp64 NU = 2 BS = 4: 148 / 0 -> 168 / 20,  168 / 200
//   fp64 NU = 2 BS = 5: 202 / 0 -> 202 / 0,   256 / 8     (bound 2 waves: 256 VGPRs)
// A kernel takes the highest level without scratch among those measured for
// its family: fp64 NU = 1 BS >= 5, the config-2 instantiation among them
// (202 VGPRs at every level), level 2, which is what the config-2 line was
// measured on; the other row-form kernels level 1 where that has
// no scratch (fp32: +10 .. 12 VGPRs at BS <= 4, none above), else the parent's loop.
#ifndef MPCQP_SETUP_UNIFORM
#define MPCQP_SETUP_UNIFORM 2
#endif
template <typename T, int NX, int NU, int BS>
struct QMpcUniform {
  static constexpr bool one = QMpcRows<T, NX, NU, BS>::v &&
                              !(sizeof(T) == 8 && (BS <= 3 || (NU == 2 && BS == 4)));
  static constexpr bool two = one && sizeof(T) == 8 && NU == 1 && BS >= 5;
  static constexpr int level =
      MPCQP_SETUP_UNIFORM >= 2 && two ? 2 : (MPCQP_SETUP_UNIFORM >= 1 && one ? 1 : 0);
};

// Row ownership of the box active set (RowOwn, gi_box_core.hpp) per instantiation.
// fp64 NX = 4 NU = 2 BS = 5 sits at 256 VGPRs either way and its scratch would
// grow from 52 to 56 bytes per lane: it keeps the replicated vectors.
template <typename T, int NX, int NU, class Mat>
struct QMpcOwned {
  static constexpr bool v =
      QRowOwned<Mat>::v && !(sizeof(T) == 8 && NX == 4 && NU == 2 && Mat::RPL == 5);
};

// Keyed reductions (Key, gi_box_core.hpp) per instantiation.  fp64 NX = 4 NU = 2 BS = 4
// sits at 256 VGPRs and its scratch would grow from 52 to 60 bytes per lane:
// it keeps the compare-and-select reductions.
template <typename T, int NX, int NU, class Mat>
struct QMpcKeyed {
  static constexpr bool v = !(sizeof(T) == 8 && NX == 4 && NU == 2 && Mat::RPL == 4);
};

// The full-step trip, the ratio filter and the bound read-ahead (RowOwn's TRIP,
// gi_box_core.hpp) per instantiation; they exist on keyed rows only.
template <typename T, int NX, int NU, class Mat>
struct QMpcTrip {
  static constexpr bool v = true;
};

template <typename T, int NX, int NU, class Mat>
struct QMpcLds {
  static constexpr bool ROWS = QMpcRows<T, NX, NU, Mat::RPL>::v;
  // oW: the W~ tile, column c at oW + c*ld, all Mat::NV rows written.  Row
  // form: the 16 lanes of a group store consecutive rows of one column.
  // Column form: each lane stores one row of its own column; ld is odd, so
  // the 16 lanes (8-byte stores, 32 four-byte banks) hit 16 distinct bank
  // pairs.  The Gram product reads a lane's BS rows of one column
  // contiguously (mpc_factor.hpp).  oK, oSi, oAcl, oX: K_k, S_k^-1, A_k + B_k K_k
  // and x-bar for the second loop of the two-loop setup (empty in row form).
  int oA, oB, oQ, oQf, oR, oC, oX0, oK, oSi, oAcl, oX, oW, total, ld;
  __host__ __device__ QMpcLds(int N, int n, int tv) {
    const int S = tv ? N : 1;
    const int N2 = ROWS ? 0 : N;
    oA = BoxLds<Mat>::oEnd;
    oB = oA + S * NX * NX;
    oQ = oB + S * NX * NU;
    oQf = oQ + NX * NX;
    oR = oQf + NX * NX;
    oC = oR + NU * NU;
    oX0 = oC + N * NX;
    oK = oX0 + NX;
    oSi = oK + N2 * NU * NX;
    oAcl = oSi + N2 * NU * NU;
    oX = oAcl + N2 * NX * NX;
    oW = oX + (ROWS ? 0 : (N + 1) * NX);
    ld = Mat::NV + 1;
    total = (oW + n * ld + 1) & ~1;  // keep every group's base 16-byte aligned
  }
};

template <typename T, int NX, int NU>
__device__ __forceinline__ void load_sq(const T* s, T (&m)[NX][NU], int ld) {
#pragma unroll
  for (int i = 0; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < NU; ++j) m[i][j] = s[i * ld + j];
}

template <typename T, int NX, int BS>
struct QMpcOcc {
  static constexpr int w = NX <= 2 ? QuadOcc<T, BS>::w : (QuadOcc<T, BS>::w < 2 ? 1 : 2);
};

// GL lanes per QP (16 with QSym: four QPs per wave); OCC: minimum waves per
// SIMD the register allocation must allow.  Measured and rejected: two QPs
// per wave (32-lane groups, 3 x 5 blocks at n = 20, row-block reductions
// through v_permlane16_swap): 73.1 vs 70.6 us at config 2 -- the per-wave
// fixed work (Riccati, x-bar/adjoint chains, reductions) doubles per QP, so
// VALU instructions per QP rose 47 % (PMC SQ_INSTS_VALU) while the two waves
// per SIMD hid only part of it.
#ifdef MPCQP_WAVE_CLOCK
// Debug library only (tools/wave_clock.py): per wave of mpc_group_kernel, the
// s_memrealtime (100 MHz, chip-wide) at entry and at exit and the largest GI
// iteration count of the wave's QPs -- the distribution of wave end times
// against the kernel's slowest wave.
constexpr int kWaveClockMax = 16384;
__device__ unsigned long long mpcqp_wave_clock[3 * kWaveClockMax];
#endif

template <typename T, int NX, int NU, class Mat, int GL, int OCC>
__global__ __launch_bounds__(64, OCC) void mpc_group_kernel(MpcArgsQ<T> a) {
#ifdef MPCQP_WAVE_CLOCK
  const unsigned long long wclk0 = __builtin_amdgcn_s_memrealtime();
#endif
  using BL = BoxLds<Mat>;
  constexpr int NV = BL::NV;
  constexpr int RPL = Mat::RPL;
  constexpr int GPW = kWave / GL;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x, g = lane / GL, q = lane % GL;
  const int b = blockIdx.x * GPW + g;
  const bool live = b < a.batch;
  const int bl = live ? b : 0;
  const int nx = a.nx, nu = a.nu, N = a.N, n = N * nu, tv = a.tv;
  const int S = tv ? N : 1;
  const QMpcLds<T, NX, NU, Mat> L(N, n, tv);
  T* sm = reinterpret_cast<T*>(smem_raw) + g * L.total;
  T* gb = sm + BL::oBuf;
  T* fs = sm + BL::oF;
  T* lbs = sm + BL::oLb;
  T* ubs = sm + BL::oUb;
  T* As = sm + L.oA;
  T* Bs = sm + L.oB;
  T* Qs = sm + L.oQ;
  T* Qfs = sm + L.oQf;
  T* Rs = sm + L.oR;
  T* Cs = sm + L.oC;
  T* X0s = sm + L.oX0;
  constexpr bool ROWS = QMpcRows<T, NX, NU, RPL>::v;
  constexpr bool UNIFORM = QMpcUniform<T, NX, NU, RPL>::level >= 1;
  [[maybe_unused]] constexpr bool PAIRS = QMpcUniform<T, NX, NU, RPL>::level == 2;
  [[maybe_unused]] T* Ks = sm + L.oK;
  [[maybe_unused]] T* Sis = sm + L.oSi;
  [[maybe_unused]] T* Acls = sm + L.oAcl;
  [[maybe_unused]] T* Xs = sm + L.oX;
  T* Wt = sm + L.oW;
  const int ld = L.ld;

#ifdef MPCQP_PHASE_TIMING
  PhaseClock mpcqp_clk;
#endif
  // Without a drift (wave-uniform) Cs is neither filled nor read: the x-bar
  // sums start from 0, which is what they would read.
  const bool has_c = a.c != nullptr;
  // ------------------------------------------------------------- stage in
  bool nonfinite = false, badbox = false;
  {
    // Element e of each array goes to lane e % GL.  The first element per
    // lane of every array (all of them unless the plant is time-varying or
    // there is a drift) and the bounds are loaded into registers before
    // anything is stored, so the wave waits for about one HBM round trip
    // instead of one per array.
    static_assert(NX * NX <= GL && NU * NU <= GL, "one element per lane for Q, Qf, R");
    constexpr int NB = (NV + GL - 1) / GL;
    const T* Ab = a.A + (int64_t)bl * a.sA;
    const T* Bb = a.B + (int64_t)bl * a.sB;
    const T* Cb = (live && a.c) ? a.c + (int64_t)b * a.sC : nullptr;
    auto ldA = [&](int e) {
      const int s = e / (NX * NX), r = (e / NX) % NX, cc = e % NX;
      return (r < nx && cc < nx) ? Ab[(int64_t)s * nx * nx + r * nx + cc] : T(0);
    };
    auto ldB = [&](int e) {
      const int s = e / (NX * NU), r = (e / NU) % NX, cc = e % NU;
      return (r < nx && cc < nu) ? Bb[(int64_t)s * nx * nu + r * nu + cc] : T(0);
    };
    auto ldC = [&](int e) {
      const int k = e / NX, cc = e % NX;
      return (Cb && cc < nx) ? Cb[k * nx + cc] : T(0);
    };
    const int rq = q / NX, cq = q % NX;
    const bool inq = live && q < NX * NX && rq < nx && cq < nx;
    const int ru = q / NU, cu = q % NU;
    const T vA = (q < S * NX * NX) ? ldA(q) : T(0);
    const T vB = (q < S * NX * NU) ? ldB(q) : T(0);
    const T vQ = inq ? a.Q[(int64_t)b * a.sQ + rq * nx + cq] : T(0);
    const T vQf = inq ? a.Qf[(int64_t)b * a.sQf + rq * nx + cq] : T(0);
    // padded inputs get R = I so that S_k stays invertible (their B cols are 0)
    const T vR = (live && ru < nu && cu < nu) ? a.R[(int64_t)b * a.sR + ru * nu + cu]
                                               : (ru == cu ? T(1) : T(0));
    const T vC = (q < N * NX) ? ldC(q) : T(0);
    const T vX0 = (live && a.x0 && q < nx) ? a.x0[(int64_t)b * a.sX0 + q] : T(0);
    T vlb[NB], vub[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int i = q + t * GL;
      const bool v = live && i < n;
      vlb[t] = (v && a.lb) ? a.lb[(int64_t)b * a.slb + i] : -Lim<T>::inf();
      vub[t] = (v && a.ub) ? a.ub[(int64_t)b * a.sub + i] : Lim<T>::inf();
    }
    if (q < S * NX * NX) As[q] = vA;
    if (q < S * NX * NU) Bs[q] = vB;
    nonfinite |= !finite(vA) || !finite(vB);
    if (q < NX * NX) {
      Qs[q] = vQ;
      Qfs[q] = vQf;
    }
    if (q < NU * NU) Rs[q] = vR;
    if (q < N * NX && has_c) Cs[q] = vC;
    if (q < NX) X0s[q] = vX0;
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int i = q + t * GL;
      if (i < NV) {
        const bool v = live && i < n;
        lbs[i] = vlb[t];
        ubs[i] = vub[t];
        fs[i] = T(0);
        badbox |= v && (!(vlb[t] <= vub[t]) || vlb[t] == Lim<T>::inf() || vub[t] == -Lim<T>::inf());
      }
    }
    // the rest of a time-varying plant and of the drift
#pragma unroll 4
    for (int e = q + GL; e < S * NX * NX; e += GL) {
      const T v = ldA(e);
      As[e] = v;
      nonfinite |= !finite(v);
    }
#pragma unroll 4
    for (int e = q + GL; e < S * NX * NU; e += GL) {
      const T v = ldB(e);
      Bs[e] = v;
      nonfinite |= !finite(v);
    }
    if (has_c) {
#pragma unroll 4
      for (int e = q + GL; e < N * NX; e += GL) Cs[e] = ldC(e);
    }
  }
  __syncthreads();

  int code = MPCQP_STATUS_OPTIMAL;
  MPCQP_PHASE(0);
  // -------------- Riccati backward + free response forward (all lanes, regs)
  // The two recursions are independent serial chains; one loop runs Riccati
  // stage N-1-t next to x-bar stage t so that their latencies overlap (at one
  // wave per SIMD nothing else hides them).
  {
    constexpr int NCH = (NV + GL - 1) / GL;  // rows (row form) / columns of W~ per lane
    T P[NX][NX], Qr[NX][NX], Rr[NU][NU], Ar[NX][NX], Br[NX][NU], Ax[NX][NX];
    load_sq<T, NX, NX>(Qfs, P, NX);
    load_sq<T, NX, NX>(Qs, Qr, NX);
    load_sq<T, NU, NU>(Rs, Rr, NU);
    load_sq<T, NX, NX>(As, Ar, NX);
    load_sq<T, NX, NU>(Bs, Br, NU);
    load_sq<T, NX, NX>(As, Ax, NX);
    T xk[NX];
#pragma unroll
    for (int qq = 0; qq < NX; ++qq) xk[qq] = X0s[qq];
    bool ok = true;
    // Rows of W~ and of f: lane q owns rows r = q + ch*GL < NV, row r being
    // input a = r % nu of stage rt = r / nu (rt = -1 for the padding rows
    // n .. NV-1, which no stage matches: their chain stays 0).  psi is the
    // row vector Psi_j(rt)[a, :], gr / hr / xr the row's g_rt[a, :], h_rt[a]
    // and xbar_{rt+1}, each caught at the step that holds it in registers.
    // Pi, pv: y_k = Pi_k xbar_k + pi_k (pi only with a drift).
    [[maybe_unused]] int rt[NCH];
    [[maybe_unused]] bool ra1[NCH];
    [[maybe_unused]] T psi[NCH][NX], gr[NCH][NX], xr[NCH][NX], hr[NCH], Pi[NX][NX], pv[NX];
    if constexpr (ROWS) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int r = q + ch * GL;
        const int tr = r / nu;
        rt[ch] = r < n ? tr : -1;
        ra1[ch] = r - tr * nu == 1;
        hr[ch] = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) psi[ch][qq] = gr[ch][qq] = xr[ch][qq] = T(0);
      }
      load_sq<T, NX, NX>(Qfs, Pi, NX);
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) pv[qq] = T(0);
    }
    // c_t: not read without a drift.  With one, the x-bar stage reads it a
    // stage ahead, so that the wait in front of its use does not also wait
    // for the LDS stores of the stage before (NX <= 2; the NX = 4 loop has no
    // registers to spare and reads it at its use).
    constexpr bool C_AHEAD = NX <= 2;
    [[maybe_unused]] T ct[NX];
    if constexpr (C_AHEAD) {
#pragma unroll
      for (int i = 0; i < NX; ++i) ct[i] = has_c ? Cs[i] : T(0);
    }
    if constexpr (UNIFORM) {
      // The launch flags are wave-uniform: one loop per combination, chosen
      // here, so that no stage tests them (mpc_setup_loop.inc).  Without a
      // drift the read-ahead is a constant 0 and not a carried value.
      if (!has_c) {
#pragma unroll
        for (int i = 0; i < NX; ++i) ct[i] = T(0);
      }
      if (tv) {
#define MPCQP_STAGE_TV true
        if (has_c) {
#define MPCQP_STAGE_HC true
#include "mpc_setup_loop.inc"
#undef MPCQP_STAGE_HC
        } else {
#define MPCQP_STAGE_HC false
#include "mpc_setup_loop.inc"
#undef MPCQP_STAGE_HC
        }
#undef MPCQP_STAGE_TV
      } else {
#define MPCQP_STAGE_TV false
        if (has_c) {
#define MPCQP_STAGE_HC true
#include "mpc_setup_loop.inc"
#undef MPCQP_STAGE_HC
        } else {
#define MPCQP_STAGE_HC false
#include "mpc_setup_loop.inc"
#undef MPCQP_STAGE_HC
        }
#undef MPCQP_STAGE_TV
      }
    } else {
#define MPCQP_STAGE_TV tv
#define MPCQP_STAGE_HC has_c
      for (int t = 0; t < N; ++t)
#include "mpc_setup_stage.inc"
#undef MPCQP_STAGE_HC
#undef MPCQP_STAGE_TV
    }
    if (!ok) code = MPCQP_STATUS_NOT_CONVEX;

    MPCQP_PHASE(1);
    if constexpr (ROWS) {
      // f_(t,a) = g_t[a, :] xbar_{t+1} + h_t[a] for the lane's own rows (the rows
      // n .. NV-1 keep the 0 of the stage-in)
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        T s = hr[ch];
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(gr[ch][qq], xr[ch][qq], s);
        if (rt[ch] >= 0) fs[q + ch * GL] = s;
      }
    } else {
      // ---- columns of W~ (forward, lockstep) next to the adjoint y -> f
      // (backward).  Lane q rolls column c = q (and c = q + GL when n > GL) of
      // W~ (mpc_factor.hpp): with v_t = L_j[:, b] at the column's own stage
      // t = j and 0 elsewhere,
      //     u_t = K_t x_t + v_t,   x_{t+1} = (A_t + B_t K_t) x_t + B_t v_t,
      // which is 0 before stage j, the start at j and the closed loop after it.
      // Every lane is at the same stage, so Ks, Acls and Bs are broadcast reads.
      // The adjoint is group-uniform and independent of the rollouts: stage
      // N-1-t runs next to rollout stage t so that the two chains overlap; its
      // x_k of the next stage is read from LDS one iteration ahead.
      __syncthreads();
      bool cv[NCH];  // NCH: columns per lane here
      int cj[NCH];
      T lj[NCH][NU], wx[NCH][NX];
      T* Wc[NCH];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c = q + ch * GL;
        cv[ch] = c < n;
        const int cc = cv[ch] ? c : 0;
        const int jj = cc / nu;
        cj[ch] = cv[ch] ? jj : -1;
        chol_col<T, NU>(Sis + jj * NU * NU, cc - jj * nu, lj[ch]);
        Wc[ch] = Wt + cc * ld;
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) wx[ch][qq] = T(0);
      }
      T yk[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        T s = T(0);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) s = fma(Qfs[i * NX + qq], xk[qq], s);
        yk[i] = s;
      }
      T xnext[NX];
#pragma unroll
      for (int qq = 0; qq < NX; ++qq) xnext[qq] = Xs[(N - 1) * NX + qq];
      // B of the rollout stage (Br) and of the adjoint stage (Ba) and A of the
      // adjoint stage (Ar) stay in registers for the whole loop unless the
      // plant is time-varying.  Every LDS read of an iteration is issued at its
      // top, before its stores (which the compiler must assume alias them);
      // K, A + B K and x-bar are read one stage ahead, after the time-varying
      // reads so that a counted wait for those leaves them in flight.  With an
      // invariant plant no stage waits for a read it has just issued.
      T Ba[NX][NU], Kt[NU][NX], Act[NX][NX];
      load_sq<T, NX, NU>(Bs, Br, NU);
      load_sq<T, NX, NU>(Bs, Ba, NU);
      load_sq<T, NU, NX>(Ks, Kt, NX);
      load_sq<T, NX, NX>(Acls, Act, NX);
      for (int t = 0; t < N; ++t) {
        const int k = N - 1 - t;  // adjoint stage
        if (tv) {
          load_sq<T, NX, NU>(Bs + t * NX * NU, Br, NU);
          load_sq<T, NX, NU>(Bs + k * NX * NU, Ba, NU);
          load_sq<T, NX, NX>(As + k * NX * NX, Ar, NX);
        }
        const int tn = t + 1 < N ? t + 1 : t;
        T Kn[NU][NX], Acn[NX][NX], xnn[NX];
        load_sq<T, NU, NX>(Ks + tn * NU * NX, Kn, NX);
        load_sq<T, NX, NX>(Acls + tn * NX * NX, Acn, NX);
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) xnn[qq] = Xs[(k > 1 ? k - 1 : 1) * NX + qq];
        {  // rollout stage t
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const bool at = t == cj[ch];
            T v[NU], u[NU], xn[NX];
#pragma unroll
            for (int i = 0; i < NU; ++i) {
              v[i] = at ? lj[ch][i] : T(0);
              T s = v[i];
#pragma unroll
              for (int qq = 0; qq < NX; ++qq) s = fma(Kt[i][qq], wx[ch][qq], s);
              u[i] = s;
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) {
              T s = T(0);
#pragma unroll
              for (int qq = 0; qq < NX; ++qq) s = fma(Act[i][qq], wx[ch][qq], s);
#pragma unroll
              for (int qq = 0; qq < NU; ++qq) s = fma(Br[i][qq], v[qq], s);
              xn[i] = s;
            }
#pragma unroll
            for (int qq = 0; qq < NX; ++qq) wx[ch][qq] = xn[qq];
            // every row is written, the zeros before stage j included
            if (cv[ch]) {
#pragma unroll
              for (int i = 0; i < NU; ++i)
                if (i < nu) Wc[ch][t * nu + i] = u[i];
            }
          }
        }
        // adjoint stage k: f_(k,u) = B_k[:,u]' y_{k+1}, then y_k
        if (q == 0) {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            T s = T(0);
#pragma unroll
            for (int qq = 0; qq < NX; ++qq) s = fma(Ba[qq][u], yk[qq], s);
            if (u < nu) fs[k * nu + u] = s;
          }
        }
        if (k > 0) {
          T yn[NX];
#pragma unroll
          for (int i = 0; i < NX; ++i) {
            T s = T(0);
#pragma unroll
            for (int qq = 0; qq < NX; ++qq) s = fma(Qr[i][qq], xnext[qq], s);
#pragma unroll
            for (int qq = 0; qq < NX; ++qq) s = fma(Ar[qq][i], yk[qq], s);
            yn[i] = s;
          }
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) yk[qq] = yn[qq];
        }
        // next stage's operands
#pragma unroll
        for (int i = 0; i < NU; ++i)
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) Kt[i][qq] = Kn[i][qq];
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
          for (int qq = 0; qq < NX; ++qq) Act[i][qq] = Acn[i][qq];
#pragma unroll
        for (int qq = 0; qq < NX; ++qq) xnext[qq] = xnn[qq];
      }
      // rows n .. NV-1 of the lane's columns: the padding of the register layout
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if (cv[ch])
          for (int i = n; i < NV; ++i) Wc[ch][i] = T(0);
    }
  }
  __syncthreads();

  MPCQP_PHASE(2);
  // ------------------------------------------------ M = -W~ W~' = -H^{-1}
  Mat M;
  M.init(lane);
  neg_gram<T>(M, Wt, ld, n);
  MPCQP_PHASE(3);
  // ---------------------------------------------------------- box QP on M
  for (int i = q; i < n; i += GL) nonfinite |= !finite(fs[i]);
  const unsigned long long gmask = (GL == 64 ? ~0ull : ((1ull << GL) - 1)) << (GL * g);
  if ((__ballot(nonfinite) & gmask) != 0) code = MPCQP_STATUS_NONFINITE;
  else if ((__ballot(badbox) & gmask) != 0) code = MPCQP_STATUS_INFEASIBLE;
  T zr[RPL];
  int iters = 0;
  using Own = RowOwn<Mat, QMpcOwned<T, NX, NU, Mat>::v, QMpcKeyed<T, NX, NU, Mat>::v,
                     QMpcTrip<T, NX, NU, Mat>::v>;
  const int c2 = gi_box<Own>(M, gb, fs, lbs, ubs, n, a.max_iter, a.tol,
                             live && code == MPCQP_STATUS_OPTIMAL, zr, iters MPCQP_CLK_ARG);
  if (code == MPCQP_STATUS_OPTIMAL) code = c2;
  MPCQP_PHASE(4);
#ifdef MPCQP_PHASE_TIMING
  mpcqp_clk.flush();
#endif
  if (code != MPCQP_STATUS_OPTIMAL && code != MPCQP_STATUS_MAXITER) {
#pragma unroll
    for (int r = 0; r < RPL; ++r) zr[r] = __builtin_nan("");
  }
  if (live && M.bj == 0) {
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      const int i = M.bi * RPL + r;
      if (i < n) a.z[(int64_t)b * n + i] = zr[r];
    }
  }
  if (live && q == 0) a.status[b] = (code & 0xff) | ((iters & 0xffff) << 8);
#ifdef MPCQP_WAVE_CLOCK
  {
    int itmax = 0;
#pragma unroll
    for (int gg = 0; gg < GPW; ++gg) {
      const int v = __builtin_amdgcn_readlane(iters, gg * GL);
      itmax = v > itmax ? v : itmax;
    }
    const unsigned long long wclk1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0 && blockIdx.x < kWaveClockMax) {
      mpcqp_wave_clock[3 * blockIdx.x] = wclk0;
      mpcqp_wave_clock[3 * blockIdx.x + 1] = wclk1;
      mpcqp_wave_clock[3 * blockIdx.x + 2] = (unsigned long long)itmax;
    }
  }
#endif
}

// ------------------------------------------------------------- launchers
template <typename T, int BS>
int launch_box_quad(const BoxArgsQ<T>& a, hipStream_t st) {
  using L = BoxLds<QSym<T, BS>>;
  constexpr int NMAX = L::NMAX;
  const size_t bytes = (size_t)4 * (L::oEnd + NMAX * (NMAX + 1) / 2) * sizeof(T);
  hipLaunchKernelGGL((box_quad_kernel<T, BS>), dim3((a.batch + 3) / 4), dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("box_quad_kernel");
  return MPCQP_OK;
}

template <typename T>
int solve_box_quad(const BoxArgsQ<T>& a, hipStream_t st) {
  return dispatch_bs<4>(a.n, [&](auto bs) {
    return launch_box_quad<T, decltype(bs)::value>(a, st);
  });
}

template <typename T, int NX, int NU, class Mat, int GL, int OCC>
int launch_mpc_group(const MpcArgsQ<T>& a, hipStream_t st) {
  constexpr int GPW = kWave / GL;
  const int n = a.N * a.nu;
  const QMpcLds<T, NX, NU, Mat> L(a.N, n, a.tv);
  const size_t bytes = (size_t)GPW * L.total * sizeof(T);
  if (bytes > 160 * 1024) {
    set_error("mpcqp_mpc_box: LDS footprint %zu B > 160 KiB", bytes);
    return MPCQP_ENOTSUP;
  }
  auto kern = mpc_group_kernel<T, NX, NU, Mat, GL, OCC>;
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kern,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(mpc_group)");
  }
  hipLaunchKernelGGL(kern, dim3((a.batch + GPW - 1) / GPW), dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("mpc_group_kernel");
  return MPCQP_OK;
}

// four QPs per wave (QSym, 16 lanes each)
template <typename T, int NX, int NU, int BS>
int launch_mpc_quad(const MpcArgsQ<T>& a, hipStream_t st) {
  return launch_mpc_group<T, NX, NU, QSym<T, BS>, 16, QMpcOcc<T, NX, BS>::w>(a, st);
}

template <typename T, int NX, int NU>
int mpc_quad_bs(const MpcArgsQ<T>& a, hipStream_t st) {
  return dispatch_bs<4>(a.N * a.nu, [&](auto bs) {
    return launch_mpc_quad<T, NX, NU, decltype(bs)::value>(a, st);
  });
}

template <typename T>
int mpc_box_quad(const MpcArgsQ<T>& a, hipStream_t st) {
  if (a.nx <= 2 && a.nu == 1) return mpc_quad_bs<T, 2, 1>(a, st);
  if (a.nx <= 2) return mpc_quad_bs<T, 2, 2>(a, st);
  if (a.nu == 1) return mpc_quad_bs<T, 4, 1>(a, st);
  return mpc_quad_bs<T, 4, 2>(a, st);
}

template int solve_box_quad<double>(const BoxArgsQ<double>&, hipStream_t);
template int solve_box_quad<float>(const BoxArgsQ<float>&, hipStream_t);
template int mpc_box_quad<double>(const MpcArgsQ<double>&, hipStream_t);
template int mpc_box_quad<float>(const MpcArgsQ<float>&, hipStream_t);

}  // namespace mpcqp

#ifdef MPCQP_WAVE_CLOCK
extern "C" int mpcqp_debug_wave_clock(unsigned long long* out, int waves) {
  const int w = waves < mpcqp::kWaveClockMax ? waves : mpcqp::kWaveClockMax;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(mpcqp::mpcqp_wave_clock),
                             3 * (size_t)w * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif

#ifdef MPCQP_PHASE_TIMING
// Debug library only: read (and optionally reset) the phase counters.
MPCQP_DEBUG_PHASE_READER(mpcqp_debug_phase_cycles)
#endif
