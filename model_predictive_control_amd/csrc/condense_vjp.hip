// condense_vjp.hip -- the adjoint of the condensing recursion
// (mpcqp_condense_vjp, include/mpcqp_diff.h): from dL/dH (packed), dL/dF and
// dL/df the gradients of the plant A, B, c, of the weights Q, R, Qf and of x0.
//
// With n = N nu and C = n + nx + 1 the forward is one recursion on the
// stacked block rows S_k = [Gam_k, Phi_k, xbar_k] (nx x C):
//     S_{-1} = [0, I, x0],   S_k = A_k S_{k-1} + E_k,
//     E_k = [B_k in column block k, 0, c_k],
//     Y = sum_k Gam_k' Q_k S_k = [H - Rhat, F, f],   Q_k = Q (k < N-1), Qf (k = N-1)
// and with GY = [Ghat, gF, gf] (n x C; Ghat symmetric, Ghat_ii = gH_ii,
// Ghat_ij = gH_ij / 2) the loss is <GY, Y> + <Ghat, Rhat>.  In reverse:
//     P_k   = Gam_k GY                                   (nx x C)
//     T_k   = P_k S_k'                                   -> gQf (k = N-1), gQ += (k < N-1)
//     GS_k  = Q_k' P_k;   GS_k[:, 0..n) += Q_k (S_k GY')
//     Lam_k = GS_k + A_{k+1}' Lam_{k+1}                  (Lam_N = 0)
//     gA_k  = Lam_k S_{k-1}',  gB_k = Lam_k[:, block k],  gc_k = Lam_k[:, last]
//     gx0 = (A_0' Lam_0)[:, last],   gR = sum_k Ghat[block k, block k]
// Ghat is symmetric, so the first n columns of the row-wise product S_k GY'
// are those of P_k: (S_k GY')[:, j] = P_k[:, j] + S_k[:, n..C) GY[j, n..C)'
// for j < n -- nx + 1 more terms per lane, no second pass over GY.
//
// Mapping: one instance per wavefront, lane j < C owns column j of S_k, P_k,
// Lam_k and GY.  The block rows S_k of the forward pass and GY stay in LDS
// (S_k[:, i] is read wave-uniformly for P_k; Gam_k has only (k+1) nu non-zero
// columns, which bounds that loop); A_k, B_k, Q, Qf are read wave-uniformly
// from LDS.  The products over the columns (T_k, gA_k) are sums across lanes:
// every lane keeps its own term of gQ, gQf and of an LTI gA in registers over
// the whole recursion, and ONE pass through LDS at the end adds the C terms of
// each entry in lane order.  With MPCQP_TV the Lam_k go to LDS and the N nx nx
// entries of gA are summed after the recursion, one entry per lane.  No
// atomics: every sum has a fixed order, so a replay gives identical bits.
#include "common.hpp"

#include "../../include/mpcqp_diff.h"

// Gam_k GY over the (k+1) nu non-zero columns of Gam_k only; 0 sums over all n
// (A/B builds: the rest of Gam_k is exact zeros, so the results are the same)
#ifndef MPCQP_CONDENSE_VJP_CAUSAL
#define MPCQP_CONDENSE_VJP_CAUSAL 1
#endif

namespace mpcqp {

constexpr int kCondVjpMaxNx = 4;
constexpr int kCondVjpMaxNu = 2;
constexpr int kCondVjpMaxN = 32;  // n = N * nu

// c, x0 and every upstream gradient, output and vstatus may be null
template <typename T>
struct CondenseVjpArgs {
  int batch, nx, nu, N, tv;
  const T* A; int64_t sA;
  const T* B; int64_t sB;
  const T* Q; int64_t sQ;
  const T* R; int64_t sR;
  const T* Qf; int64_t sQf;
  const T* c; int64_t sC;
  const T* x0; int64_t sX0;
  const T *gH, *gF, *gf;
  T *gA, *gB, *gQ, *gR, *gQf, *gc, *gx0;
  int32_t* vstatus;
};

// Per-instance LDS (elements).  S holds N + 1 block rows, slot k + 1 = S_k and
// slot 0 = S_{-1}; Lam (MPCQP_TV with gA only) the N block rows Lam_k.  The
// scratch of the final sums (3 nx nx rows of C lane terms) overlays S and Lam,
// which are dead by then.
struct VLayout {
  int oA, oB, oQ, oQf, oC, oX0, oGY, oBv, oS, oLam, oRed, total;
};
__host__ __device__ inline VLayout vlayout(int NX, int nu, int N, int tv, int lam) {
  VLayout L;
  const int n = N * nu, C = n + NX + 1, S = tv ? N : 1;
  int o = 0;
  L.oA = o; o += S * NX * NX;
  L.oB = o; o += S * NX * nu;
  L.oQ = o; o += NX * NX;
  L.oQf = o; o += NX * NX;
  L.oC = o; o += N * NX;
  L.oX0 = o; o += NX;
  L.oGY = o; o += n * C;
  L.oBv = o; o += NX * n;
  L.oS = o; o += (N + 1) * NX * C;
  L.oLam = o; o += lam ? N * NX * C : 0;
  L.oRed = L.oS;
  const int red = L.oRed + 3 * NX * NX * C;
  L.total = o > red ? o : red;
  return L;
}

// row of element e of a packed lower triangle (e < 2^20)
__device__ __forceinline__ int packed_row(int e) {
  int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
  i -= (i * (i + 1) / 2 > e) ? 1 : 0;
  i += ((i + 1) * (i + 2) / 2 <= e) ? 1 : 0;
  return i;
}

template <typename T, int NX>
__global__ __launch_bounds__(64) void condense_vjp_kernel(CondenseVjpArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* sm = reinterpret_cast<T*>(smem_raw);
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int nu = a.nu, N = a.N, n = N * nu, tv = a.tv;
  const int C = n + NX + 1;
  const int SA = tv ? N : 1;
  const bool lamLds = tv && a.gA;
  const VLayout L = vlayout(NX, nu, N, tv, lamLds ? 1 : 0);
  T* As = sm + L.oA;
  T* Bs = sm + L.oB;
  T* Qs = sm + L.oQ;
  T* Qfs = sm + L.oQf;
  T* Cs = sm + L.oC;
  T* X0s = sm + L.oX0;
  T* GYs = sm + L.oGY;
  T* Bvs = sm + L.oBv;
  T* Ss = sm + L.oS;
  T* Lams = sm + L.oLam;
  T* Red = sm + L.oRed;

  // ------------------------------------------------------------- stage in
  // every input of the instance and every given upstream row is looked at
  bool nonfinite = false;
  auto stage = [&](T* dst, const T* src, int cnt) {
    for (int e = lane; e < cnt; e += kWave) {
      const T v = src ? src[e] : T(0);
      nonfinite |= !finite(v);
      dst[e] = v;
    }
  };
  stage(As, a.A + (int64_t)b * a.sA, SA * NX * NX);
  stage(Bs, a.B + (int64_t)b * a.sB, SA * NX * nu);
  stage(Qs, a.Q + (int64_t)b * a.sQ, NX * NX);
  stage(Qfs, a.Qf + (int64_t)b * a.sQf, NX * NX);
  stage(Cs, a.c ? a.c + (int64_t)b * a.sC : nullptr, N * NX);
  stage(X0s, a.x0 ? a.x0 + (int64_t)b * a.sX0 : nullptr, NX);
  {
    const T* Rb = a.R + (int64_t)b * a.sR;  // R enters H additively: its gradient needs no value
    if (lane < nu * nu) nonfinite |= !finite(Rb[lane]);
  }
  {
    const int P = n * (n + 1) / 2;
    const T* gHb = a.gH ? a.gH + (int64_t)b * P : nullptr;
    for (int e = lane; e < P; e += kWave) {
      const int i = packed_row(e), j = e - i * (i + 1) / 2;
      T v = gHb ? gHb[e] : T(0);
      nonfinite |= !finite(v);
      v = (i == j) ? v : T(0.5) * v;
      GYs[i * C + j] = v;
      GYs[j * C + i] = v;
    }
    const T* gFb = a.gF ? a.gF + (int64_t)b * n * NX : nullptr;
    for (int e = lane; e < n * NX; e += kWave) {
      const int i = e / NX, q = e - i * NX;
      const T v = gFb ? gFb[e] : T(0);
      nonfinite |= !finite(v);
      GYs[i * C + n + q] = v;
    }
    const T* gfb = a.gf ? a.gf + (int64_t)b * n : nullptr;
    for (int i = lane; i < n; i += kWave) {
      const T v = gfb ? gfb[i] : T(0);
      nonfinite |= !finite(v);
      GYs[i * C + n + NX] = v;
    }
  }
  T* gAb = a.gA ? a.gA + (int64_t)b * SA * NX * NX : nullptr;
  T* gBb = a.gB ? a.gB + (int64_t)b * SA * NX * nu : nullptr;
  T* gQb = a.gQ ? a.gQ + (int64_t)b * NX * NX : nullptr;
  T* gQfb = a.gQf ? a.gQf + (int64_t)b * NX * NX : nullptr;
  T* gRb = a.gR ? a.gR + (int64_t)b * nu * nu : nullptr;
  T* gcb = a.gc ? a.gc + (int64_t)b * N * NX : nullptr;
  T* gx0b = a.gx0 ? a.gx0 + (int64_t)b * NX : nullptr;
  const bool bad = __ballot(nonfinite) != 0;  // uniform: the wavefront is the instance
  if (lane == 0 && a.vstatus) a.vstatus[b] = bad ? MPCQP_STATUS_NONFINITE : MPCQP_STATUS_OPTIMAL;
  if (bad) {
    auto zero = [&](T* dst, int cnt) {
      if (dst)
        for (int e = lane; e < cnt; e += kWave) dst[e] = T(0);
    };
    zero(gAb, SA * NX * NX);
    zero(gBb, SA * NX * nu);
    zero(gQb, NX * NX);
    zero(gQfb, NX * NX);
    zero(gRb, nu * nu);
    zero(gcb, N * NX);
    zero(gx0b, NX);
    return;
  }
  wave_lds_sync();

  // ------------------------------------------------- forward: the block rows S_k
  // lanes past the last column repeat it; they write nothing
  const bool act = lane < C;
  const int j = act ? lane : C - 1;
  const bool isz = j < n;
  const bool last = j == C - 1;
  const int jb = isz ? j / nu : -1;       // the stage of a z column
  const int ja = isz ? j - jb * nu : 0;   // and its input
  {
    T s[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) s[q] = last ? X0s[q] : ((!isz && j - n == q) ? T(1) : T(0));
    if (act)
#pragma unroll
      for (int q = 0; q < NX; ++q) Ss[q * C + j] = s[q];
    for (int k = 0; k < N; ++k) {
      const T* Ak = As + (tv ? k : 0) * NX * NX;
      const T* Bk = Bs + (tv ? k : 0) * NX * nu;
      const bool inj = isz && jb == k;
      T t[NX];
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        T acc = last ? Cs[k * NX + r] : (inj ? Bk[r * nu + ja] : T(0));
#pragma unroll
        for (int q = 0; q < NX; ++q) acc = fma(Ak[r * NX + q], s[q], acc);
        t[r] = acc;
      }
#pragma unroll
      for (int q = 0; q < NX; ++q) s[q] = t[q];
      if (act)
#pragma unroll
        for (int q = 0; q < NX; ++q) Ss[((k + 1) * NX + q) * C + j] = s[q];
    }
  }
  wave_lds_sync();

  // ------------------------------------------------------------- reverse
  T gyr[NX + 1];  // GY[j, n..C) of a z column's own row
#pragma unroll
  for (int c = 0; c < NX + 1; ++c) gyr[c] = GYs[(isz ? j : 0) * C + n + c];
  T lam[NX], bsv[NX], tQ[NX][NX], tQf[NX][NX], tA[NX][NX];
#pragma unroll
  for (int q = 0; q < NX; ++q) {
    lam[q] = bsv[q] = T(0);
#pragma unroll
    for (int r = 0; r < NX; ++r) tQ[q][r] = tQf[q][r] = tA[q][r] = T(0);
  }
  for (int k = N - 1; k >= 0; --k) {
    const T* Sk = Ss + (k + 1) * NX * C;
    const T* Sp = Ss + k * NX * C;
    const T* Qk = (k == N - 1) ? Qfs : Qs;
    T P[NX], sk[NX], sp[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      P[q] = T(0);
      sk[q] = Sk[q * C + j];
      sp[q] = Sp[q * C + j];
    }
    const int w = MPCQP_CONDENSE_VJP_CAUSAL ? (k + 1) * nu : n;  // the non-zero columns of Gam_k
    for (int i = 0; i < w; ++i) {
      const T g = GYs[i * C + j];
#pragma unroll
      for (int q = 0; q < NX; ++q) P[q] = fma(Sk[q * C + i], g, P[q]);
    }
    T V[NX];  // column j < n of S_k GY'
#pragma unroll
    for (int p = 0; p < NX; ++p) {
      T acc = P[p];
#pragma unroll
      for (int c = 0; c < NX + 1; ++c) acc = fma(Sk[p * C + n + c], gyr[c], acc);
      V[p] = isz ? acc : T(0);
    }
    T nl[NX];
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      T acc = T(0);
#pragma unroll
      for (int p = 0; p < NX; ++p) acc = fma(Qk[p * NX + q], P[p], acc);
#pragma unroll
      for (int p = 0; p < NX; ++p) acc = fma(Qk[q * NX + p], V[p], acc);
      nl[q] = acc;
    }
    if (k < N - 1) {
      const T* A1 = As + (tv ? k + 1 : 0) * NX * NX;
#pragma unroll
      for (int q = 0; q < NX; ++q)
#pragma unroll
        for (int p = 0; p < NX; ++p) nl[q] = fma(A1[p * NX + q], lam[p], nl[q]);
    }
#pragma unroll
    for (int q = 0; q < NX; ++q) lam[q] = nl[q];
#pragma unroll
    for (int q = 0; q < NX; ++q)
#pragma unroll
      for (int r = 0; r < NX; ++r) tQ[q][r] = fma(P[q], sk[r], tQ[q][r]);
    if (k == N - 1) {
#pragma unroll
      for (int q = 0; q < NX; ++q)
#pragma unroll
        for (int r = 0; r < NX; ++r) {
          tQf[q][r] = tQ[q][r];
          tQ[q][r] = T(0);
        }
    }
    if (lamLds) {
      if (act)
#pragma unroll
        for (int q = 0; q < NX; ++q) Lams[(k * NX + q) * C + j] = lam[q];
    } else {
#pragma unroll
      for (int q = 0; q < NX; ++q)
#pragma unroll
        for (int r = 0; r < NX; ++r) tA[q][r] = fma(lam[q], sp[r], tA[q][r]);
    }
    if (isz && jb == k)
#pragma unroll
      for (int q = 0; q < NX; ++q) bsv[q] = lam[q];
    if (gcb && last && act)
#pragma unroll
      for (int q = 0; q < NX; ++q) gcb[k * NX + q] = lam[q];
  }
  if (gx0b && last && act) {
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      T acc = T(0);
#pragma unroll
      for (int p = 0; p < NX; ++p) acc = fma(As[p * NX + q], lam[p], acc);  // A_0
      gx0b[q] = acc;
    }
  }

  // ------------------------------------------------ gB, gR, time-varying gA
  if (isz && act)
#pragma unroll
    for (int q = 0; q < NX; ++q) Bvs[q * n + j] = bsv[q];
  wave_lds_sync();
  if (gBb) {
    if (tv) {
      for (int e = lane; e < N * NX * nu; e += kWave) {
        const int k = e / (NX * nu), rem = e - k * NX * nu;
        const int q = rem / nu, aa = rem - q * nu;
        gBb[e] = Bvs[q * n + k * nu + aa];
      }
    } else if (lane < NX * nu) {
      const int q = lane / nu, aa = lane - q * nu;
      T acc = T(0);
      for (int k = 0; k < N; ++k) acc += Bvs[q * n + k * nu + aa];
      gBb[lane] = acc;
    }
  }
  if (gRb && lane < nu * nu) {
    const int aa = lane / nu, bb = lane - aa * nu;
    T acc = T(0);
    for (int k = 0; k < N; ++k) acc += GYs[(k * nu + aa) * C + k * nu + bb];
    gRb[lane] = acc;
  }
  if (lamLds) {
    for (int e = lane; e < N * NX * NX; e += kWave) {
      const int k = e / (NX * NX), rem = e - k * NX * NX;
      const int q = rem / NX, r = rem - q * NX;
      const T* Lk = Lams + (k * NX + q) * C;
      const T* Sr = Ss + (k * NX + r) * C;  // slot k = S_{k-1}
      T acc = T(0);
      for (int c = 0; c < C; ++c) acc = fma(Lk[c], Sr[c], acc);
      gAb[e] = acc;
    }
  }
  wave_lds_sync();  // S and Lam are dead: the lane terms take their place

  // --------------------------------------- the sums over the lanes: gQ, gQf, gA
  if (act) {
#pragma unroll
    for (int q = 0; q < NX; ++q)
#pragma unroll
      for (int r = 0; r < NX; ++r) {
        const int e = q * NX + r;
        Red[e * C + j] = tQ[q][r];
        Red[(NX * NX + e) * C + j] = tQf[q][r];
        Red[(2 * NX * NX + e) * C + j] = tA[q][r];
      }
  }
  wave_lds_sync();
  if (lane < 3 * NX * NX) {
    const int m = lane / (NX * NX), e = lane - m * NX * NX;
    const int q = e / NX, r = e - q * NX;
    const T* R1 = Red + (m * NX * NX + q * NX + r) * C;
    const T* R2 = Red + (m * NX * NX + r * NX + q) * C;
    T s1 = T(0), s2 = T(0);
    for (int c = 0; c < C; ++c) {
      s1 += R1[c];
      s2 += R2[c];
    }
    // the weights' gradients symmetrised, as mpc_box_diff returns them
    if (m == 0 && gQb) gQb[e] = T(0.5) * (s1 + s2);
    if (m == 1 && gQfb) gQfb[e] = T(0.5) * (s1 + s2);
    if (m == 2 && gAb && !tv) gAb[e] = s1;
  }
}

template <typename T, int NX>
static int launch_condense_vjp(const CondenseVjpArgs<T>& a, hipStream_t st) {
  const size_t bytes =
      (size_t)vlayout(NX, a.nu, a.N, a.tv, (a.tv && a.gA) ? 1 : 0).total * sizeof(T);
  if (bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)condense_vjp_kernel<T, NX>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(condense_vjp)");
  }
  hipLaunchKernelGGL((condense_vjp_kernel<T, NX>), dim3(a.batch), dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("condense_vjp_kernel");
  return MPCQP_OK;
}

}  // namespace mpcqp

// The argument checks, all before any device work.
extern "C" int mpcqp_condense_vjp(int dtype, int batch, int nx, int nu, int N, int flags,
                                  const void* A, int64_t strideA, const void* Bm, int64_t strideB,
                                  const void* Q, int64_t strideQ, const void* R, int64_t strideR,
                                  const void* Qf, int64_t strideQf, const void* c, int64_t strideC,
                                  const void* x0, int64_t strideX0, const void* gH, const void* gF,
                                  const void* gf, void* gA, void* gB, void* gQ, void* gR, void* gQf,
                                  void* gc, void* gx0, int32_t* vstatus, void* stream) {
  using namespace mpcqp;
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "mpcqp_condense_vjp: bad dtype %d",
                  dtype);
  MPCQP_CHECK_ARG(batch >= 0, "mpcqp_condense_vjp: batch < 0");
  MPCQP_CHECK_ARG((flags & ~MPCQP_TV) == 0,
                  "mpcqp_condense_vjp: flags=%d: only MPCQP_TV is accepted", flags);
  // the limits of mpcqp_condense
  MPCQP_CHECK_ARG(nx >= 1 && nx <= 16, "mpcqp_condense_vjp: nx=%d outside [1,16]", nx);
  MPCQP_CHECK_ARG(nu >= 1 && nu <= 16, "mpcqp_condense_vjp: nu=%d outside [1,16]", nu);
  MPCQP_CHECK_ARG(N >= 1 && (int64_t)N * nu <= 4096, "mpcqp_condense_vjp: N=%d out of range", N);
  // those of the differentiable paths
  if (nx > kCondVjpMaxNx) {
    set_error("mpcqp_condense_vjp: nx=%d above the limit %d", nx, kCondVjpMaxNx);
    return MPCQP_ENOTSUP;
  }
  if (nu > kCondVjpMaxNu) {
    set_error("mpcqp_condense_vjp: nu=%d above the limit %d", nu, kCondVjpMaxNu);
    return MPCQP_ENOTSUP;
  }
  if (N * nu > kCondVjpMaxN) {
    set_error("mpcqp_condense_vjp: N*nu=%d above the limit %d", N * nu, kCondVjpMaxN);
    return MPCQP_ENOTSUP;
  }
  if (batch == 0) return MPCQP_OK;
  MPCQP_CHECK_ARG(A && Bm && Q && R && Qf, "mpcqp_condense_vjp: A, B, Q, R, Qf are required");
  MPCQP_CHECK_ARG(strideA >= 0 && strideB >= 0 && strideQ >= 0 && strideR >= 0 && strideQf >= 0 &&
                      strideC >= 0 && strideX0 >= 0,
                  "mpcqp_condense_vjp: negative stride");
  auto run = [&](auto tp) {
    using T = decltype(tp);
    const CondenseVjpArgs<T> a{batch, nx, nu, N, (flags & MPCQP_TV) ? 1 : 0,
                               (const T*)A, strideA, (const T*)Bm, strideB, (const T*)Q, strideQ,
                               (const T*)R, strideR, (const T*)Qf, strideQf, (const T*)c, strideC,
                               (const T*)x0, strideX0, (const T*)gH, (const T*)gF, (const T*)gf,
                               (T*)gA, (T*)gB, (T*)gQ, (T*)gR, (T*)gQf, (T*)gc, (T*)gx0, vstatus};
    hipStream_t st = (hipStream_t)stream;
    switch (nx) {
      case 1: return launch_condense_vjp<T, 1>(a, st);
      case 2: return launch_condense_vjp<T, 2>(a, st);
      case 3: return launch_condense_vjp<T, 3>(a, st);
      default: return launch_condense_vjp<T, 4>(a, st);
    }
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}
