// loop_box_vjp.hip -- mpcqp_mpc_box_loop_vjp: the adjoint of the one-launch
// box-MPC loop (loop_box.hip), the whole reverse-time recursion in ONE launch,
// four instances per wavefront on the QSym layout of quad.hpp.
//
// Forward (mpcqp_mpc_box_loop[_affine]), per instance, t = 0..T-1:
//     f_t = F x_t + g_t,   z_t = argmin 1/2 z'Hz + f_t'z over lb <= z <= ub,
//     u_t = z_t[0..nu),    x_{t+1} = A x_t + B u_t + w_t
// With L any function of xs, us, zs and gxs, gus, gzs its upstream gradients
// (each may be absent = 0):
//     lam <- gxs[T]
//     for t = T-1 .. 0:
//         gz <- gzs[t];  gz[0..nu) += gus[t] + B'lam
//         A_t = rows with z_t,i == lb_i or == ub_i (exact), F_t the rest
//         d_F = -H_FF^-1 gz_F, d_A = 0;  nu_A = gz_A + H_AF d_F    (box_vjp.hip)
//         gg[t] = d,  gw[t] = lam                        (lam is lam_{t+1} here)
//         gH += fold(d z_t'),  gF += d x_t',  gA += lam x_t',  gB += lam u_t'
//         glb += nu at lb (lb == ub == z counts as lb),  gub += nu at ub
//         lam <- gxs[t] + A'lam + F'd
//     gx0 = lam
// Everything of an instance stays on chip for the episode: packed H, F, A, B
// and the bounds are staged once into the group's LDS block, lam and the
// accumulators of gH (a packed tile), gF, glb, gub live in LDS and those of gA,
// gB in one register of their owner lane.  Every accumulator entry is updated
// by exactly one lane (no atomics) and written to HBM once, at the end.  Per
// step the kernel rebuilds M = SWEEP_F(H) from the packed tile and runs the
// step function of box_vjp_core.hpp, the one the stand-alone adjoint runs: a
// step's d and nu are those of mpcqp_solve_box_vjp on the same data and no
// round-off drifts over T.  Per step and instance only z_t, x_t
// and the given ones of gzs[t], gus[t], gxs[t] are read and gg[t], gw[t]
// written; the rows of step t-1 are loaded (into the registers step t's rows
// have just left) before step t's sweeps, so their latency lies under the
// sweep loop -- the one-step-ahead pattern of the affine loop with t descending.
//
// An instance whose outcome is not OPTIMAL gets exact zeros in every output,
// its gg and gw rows included (rewritten in the epilogue by the lanes that
// wrote them).  Division is IEEE (built without the approximate-division
// flags).
#include "box_vjp_core.hpp"
#include "quad_api.hpp"

namespace mpcqp {

template <typename T>
struct LoopVjpArgs {
  int batch, nx, nu, n, steps;
  const T* H; int64_t sH;      // packed lower n(n+1)/2 per instance
  const T* F; int64_t sF;      // n x nx
  const T* A; int64_t sA;      // nx x nx
  const T* B; int64_t sB;      // nx x nu
  const T* lb; int64_t slb;
  const T* ub; int64_t sub;
  const T* xs;                 // (steps + 1) x batch x nx (row `steps` is not read)
  const T* zs;                 // steps x batch x n
  const int32_t* status;       // steps x batch, or null
  const T* gxs;                // (steps + 1) x batch x nx, or null
  const T* gus;                // steps x batch x nu, or null
  const T* gzs;                // steps x batch x n, or null
  T *gx0, *gH, *gF, *gA, *gB, *glb, *gub;  // per instance, dense; each may be null
  T *gg, *gw;                  // steps x batch x n, steps x batch x nx; may be null
  int32_t* vstatus;
};

// Per-group LDS: the QSym exchange tile; the staged problem (packed H, F, A, B,
// bounds); the accumulators (gH as a packed tile, gF, glb, gub); the step's
// rows z, gz, d, x and lam.
template <typename T, int NX, int NU, int BS>
struct LoopVjpLds {
  static constexpr int NMAX = QSym<T, BS>::NMAX;
  static constexpr int PMAX = NMAX * (NMAX + 1) / 2;
  static constexpr int oBuf = 0;
  static constexpr int oP = QSym<T, BS>::BUF;
  static constexpr int oGH = oP + PMAX;
  static constexpr int oF = oGH + PMAX;
  static constexpr int oGF = oF + NMAX * NX;
  static constexpr int oA = oGF + NMAX * NX;
  static constexpr int oB = oA + NX * NX;
  static constexpr int oLb = oB + NX * NU;
  static constexpr int oUb = oLb + NMAX;
  static constexpr int oGlb = oUb + NMAX;
  static constexpr int oGub = oGlb + NMAX;
  static constexpr int oZ = oGub + NMAX;
  static constexpr int oG = oZ + NMAX;
  static constexpr int oD = oG + NMAX;
  static constexpr int oX = oD + NMAX;
  static constexpr int oL = oX + NX;
  static constexpr int size = (oL + NX + 1) & ~1;
};

template <typename T, int NX, int NU, int BS>
__global__ __launch_bounds__(64) void box_loop_vjp_kernel(LoopVjpArgs<T> a) {
  using L = LoopVjpLds<T, NX, NU, BS>;
  constexpr int NMAX = L::NMAX;
  constexpr int PMAX = L::PMAX;
  constexpr int RK = (NMAX + 15) / 16;  // rows q + 16 k of a row vector per lane
  static_assert(NX * NX <= 16 && NX * NU <= 16, "one lane per entry of gA and gB");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
  const int b = blockIdx.x * 4 + g;
  const bool live = b < a.batch;
  const int bl = live ? b : 0;
  const int n = a.n, nx = a.nx, nu = a.nu, P = n * (n + 1) / 2, steps = a.steps;
  T* gs = reinterpret_cast<T*>(smem_raw) + g * L::size;
  T* gb = gs + L::oBuf;
  T* Ps = gs + L::oP;
  T* GHs = gs + L::oGH;
  T* Fs = gs + L::oF;
  T* GFs = gs + L::oGF;
  T* As = gs + L::oA;
  T* Bs = gs + L::oB;
  T* lbs = gs + L::oLb;
  T* ubs = gs + L::oUb;
  T* glbs = gs + L::oGlb;
  T* gubs = gs + L::oGub;
  T* zs = gs + L::oZ;
  T* gzl = gs + L::oG;
  T* ds = gs + L::oD;
  T* xg = gs + L::oX;
  T* ls = gs + L::oL;
  // ------------------------------------------------------------- stage in
  bool nf0 = false;
  {
    const T* Hb = a.H + (int64_t)bl * a.sH;
    for (int e = q; e < PMAX; e += 16) {
      const T v = e < P ? Hb[e] : T(0);
      nf0 |= !finite(v);
      Ps[e] = v;
      GHs[e] = T(0);
    }
    const T* Fb = a.F + (int64_t)bl * a.sF;
    for (int e = q; e < NMAX * NX; e += 16) {
      const int i = e / NX, j = e - i * NX;
      const T v = (i < n && j < nx) ? Fb[i * nx + j] : T(0);
      nf0 |= !finite(v);
      Fs[e] = v;
      GFs[e] = T(0);
    }
    if (q < NX * NX) {
      const int i = q / NX, j = q - i * NX;
      const T v = (i < nx && j < nx) ? a.A[(int64_t)bl * a.sA + i * nx + j] : T(0);
      nf0 |= !finite(v);
      As[q] = v;
    }
    if (q < NX * NU) {
      const int i = q / NU, j = q - i * NU;
      const T v = (i < nx && j < nu) ? a.B[(int64_t)bl * a.sB + i * nu + j] : T(0);
      nf0 |= !finite(v);
      Bs[q] = v;
    }
    for (int i = q; i < NMAX; i += 16) {
      const bool v = live && i < n;
      lbs[i] = (v && a.lb) ? a.lb[(int64_t)b * a.slb + i] : -Lim<T>::inf();
      ubs[i] = (v && a.ub) ? a.ub[(int64_t)b * a.sub + i] : Lim<T>::inf();
      glbs[i] = T(0);
      gubs[i] = T(0);
    }
    // lam = gxs[T]
    if (q < NX) {
      const T v = (live && a.gxs && q < nx) ? a.gxs[((int64_t)steps * a.batch + b) * nx + q] : T(0);
      nf0 |= !finite(v);
      ls[q] = v;
    }
  }
  const int sh = 16 * g;
  const unsigned long long gmask = 0xFFFFull << sh;
  // The forward's own failure goes first: the code of the first step that did
  // not end OPTIMAL (it wrote NaN into z for every code but MAXITER, and
  // NONFINITE here would hide the cause).
  int fcode = MPCQP_STATUS_OPTIMAL;
  if (a.status) {
    for (int base = 0; base < steps; base += 16) {
      const int t = base + q;
      const int c = (live && t < steps) ? (a.status[(int64_t)t * a.batch + b] & 0xff)
                                        : MPCQP_STATUS_OPTIMAL;
      const unsigned m16 = (unsigned)((__ballot(c != MPCQP_STATUS_OPTIMAL) >> sh) & 0xFFFFull);
      if (fcode == MPCQP_STATUS_OPTIMAL && m16 != 0)
        fcode = a.status[(int64_t)(base + __builtin_ctz(m16)) * a.batch + b] & 0xff;
    }
  }
  __syncthreads();
  bool nonfin = live && (__ballot(nf0) & gmask) != 0;  // of the group, from here on
  bool notconv = false;

  // This lane's entries of the step's rows, loaded one step ahead: rows q and
  // q + 16 of z_t and gzs[t], entry q of x_t, gus[t] and gxs[t]; 0 where there
  // is none (a row past n, an absent gradient).
  T zn[RK], gn[RK], xn = T(0), un = T(0), sn = T(0);
#pragma unroll
  for (int k = 0; k < RK; ++k) zn[k] = gn[k] = T(0);
  auto fetch = [&](int t) {
    if (!live) return;
    const int64_t rb = (int64_t)t * a.batch + b;
#pragma unroll
    for (int k = 0; k < RK; ++k)
      if (q + 16 * k < n) {
        zn[k] = a.zs[rb * n + q + 16 * k];
        if (a.gzs) gn[k] = a.gzs[rb * n + q + 16 * k];
      }
    if (q < nx) {
      xn = a.xs[rb * nx + q];
      if (a.gxs) sn = a.gxs[rb * nx + q];
    }
    if (a.gus && q < nu) un = a.gus[rb * nu + q];
  };
  if (steps > 0) fetch(steps - 1);

  QSym<T, BS> M;
  M.init(lane);
  T accA = T(0), accB = T(0);  // gA entry q (q < NX * NX), gB entry q (q < NX * NU)

  for (int t = steps - 1; t >= 0; --t) {
    const bool first = t == steps - 1;  // the accumulators are set, not added to
    const int64_t rb = (int64_t)t * a.batch + b;
    // the step's rows into LDS: z_t, x_t, gz = gzs[t] (+ gus[t] + B'lam on the
    // first nu rows)
    bool nfr = !finite(xn) || !finite(un) || !finite(sn);
#pragma unroll
    for (int k = 0; k < RK; ++k) {
      const int i = q + 16 * k;
      nfr |= !finite(zn[k]) || !finite(gn[k]);
      T v = gn[k];
      if (k == 0 && q < NU) {
        T s = un;
#pragma unroll
        for (int j = 0; j < NX; ++j) s = fma(Bs[j * NU + q], ls[j], s);
        v += s;
      }
      if (i < NMAX) {
        gzl[i] = v;
        zs[i] = zn[k];
      }
    }
    if (q < NX) xg[q] = xn;
    const T sx = sn;  // gxs[t], for the end of the step
    nonfin = nonfin || (__ballot(nfr) & gmask) != 0;
    lds_exchange();
    // the rows of step t - 1: in flight during the sweeps below
    if (t > 0) fetch(t - 1);
    const bool run = live && fcode == MPCQP_STATUS_OPTIMAL && !nonfin && !notconv;

    // the step (box_vjp_core.hpp): d and nu from the packed tile (H was checked
    // at stage-in: the load's flag is dropped)
    bool nfh = false;
    M.load_packed(Ps, n, nfh);
    T zr[BS], dr[BS], nur[BS];
    int st[BS];
    const bool good = box_vjp_step(M, gb, zs, gzl, lbs, ubs, n, g, run, zr, st, dr, nur);
    notconv = notconv || (run && !good);
    // gg[t] = d, gw[t] = lam_{t+1}; d to LDS; glb, gub by the rows' owners
    if (M.bj == 0) {
#pragma unroll
      for (int r = 0; r < BS; ++r) {
        const int i = M.bi * BS + r;
        ds[i] = dr[r];
        const T vl = st[r] == 1 ? nur[r] : T(0), vu = st[r] == 2 ? nur[r] : T(0);
        glbs[i] = first ? vl : glbs[i] + vl;
        gubs[i] = first ? vu : gubs[i] + vu;
        if (good && a.gg && i < n) a.gg[rb * n + i] = dr[r];
      }
    }
    if (good && a.gw && q < nx) a.gw[rb * nx + q] = ls[q];
    lds_exchange();
    // gH += fold(d z')
    fold_dz(M, ds, zs, dr, zr, n, [&](int e, T v) { GHs[e] = first ? v : GHs[e] + v; });
    // gF += d x', gA += lam x', gB += lam u'
    for (int e = q; e < NMAX * NX; e += 16) {
      const int i = e / NX, j = e - i * NX;
      const T v = ds[i] * xg[j];
      GFs[e] = first ? v : GFs[e] + v;
    }
    if (q < NX * NX) accA = fma(ls[q / NX], xg[q % NX], accA);
    if (q < NX * NU) accB = fma(ls[q / NU], zs[q % NU], accB);
    // lam <- gxs[t] + A'lam + F'd
    T ln = sx;
    if (q < NX) {
#pragma unroll
      for (int i = 0; i < NX; ++i) ln = fma(As[i * NX + q], ls[i], ln);
#pragma unroll
      for (int i = 0; i < NMAX; ++i) ln = fma(Fs[i * NX + q], ds[i], ln);
    }
    lds_exchange();
    if (q < NX) ls[q] = ln;
    lds_exchange();
  }

  // ------------------------------------------------------------- epilogue
  int code = fcode;
  if (code == MPCQP_STATUS_OPTIMAL && nonfin) code = MPCQP_STATUS_NONFINITE;
  if (code == MPCQP_STATUS_OPTIMAL && notconv) code = MPCQP_STATUS_NOT_CONVEX;
  const bool ok = code == MPCQP_STATUS_OPTIMAL;
  if (!live) return;
  if (q == 0 && a.vstatus) a.vstatus[b] = code;
  if (a.gH) {
    T* o = a.gH + (int64_t)b * P;
    for (int e = q; e < P; e += 16) o[e] = ok ? GHs[e] : T(0);
  }
  if (a.gF) {
    T* o = a.gF + (int64_t)b * n * nx;
    for (int e = q; e < NMAX * NX; e += 16) {
      const int i = e / NX, j = e - i * NX;
      if (i < n && j < nx) o[i * nx + j] = ok ? GFs[e] : T(0);
    }
  }
  if (q < NX * NX) {
    const int i = q / NX, j = q % NX;
    if (a.gA && i < nx && j < nx) a.gA[(int64_t)b * nx * nx + i * nx + j] = ok ? accA : T(0);
  }
  if (q < NX * NU) {
    const int i = q / NU, j = q % NU;
    if (a.gB && i < nx && j < nu) a.gB[(int64_t)b * nx * nu + i * nu + j] = ok ? accB : T(0);
  }
  for (int i = q; i < n; i += 16) {
    if (a.glb) a.glb[(int64_t)b * n + i] = ok ? glbs[i] : T(0);
    if (a.gub) a.gub[(int64_t)b * n + i] = ok ? gubs[i] : T(0);
  }
  if (a.gx0 && q < nx) a.gx0[(int64_t)b * nx + q] = ok ? ls[q] : T(0);
  // A failure zeroes the rows of gg and gw: a failed forward or a NaN in the
  // staged data left them unwritten, a failure found mid-episode leaves the
  // rows of the later steps behind.  The lanes that wrote a row rewrite it, so
  // the two stores to an address are one lane's, in program order.
  if (!ok) {
    for (int t = 0; t < steps; ++t) {
      const int64_t rb = (int64_t)t * a.batch + b;
      if (a.gg && M.bj == 0) {
#pragma unroll
        for (int r = 0; r < BS; ++r) {
          const int i = M.bi * BS + r;
          if (i < n) a.gg[rb * n + i] = T(0);
        }
      }
      if (a.gw && q < nx) a.gw[rb * nx + q] = T(0);
    }
  }
}

template <typename T, int NX, int NU, int BS>
static int launch_loop_vjp(const LoopVjpArgs<T>& a, hipStream_t st) {
  constexpr size_t bytes = (size_t)4 * LoopVjpLds<T, NX, NU, BS>::size * sizeof(T);
  static_assert(bytes <= 64 * 1024, "the four groups' LDS blocks fit the default limit");
  hipLaunchKernelGGL((box_loop_vjp_kernel<T, NX, NU, BS>), dim3((unsigned)((a.batch + 3) / 4)),
                     dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("box_loop_vjp_kernel");
  return MPCQP_OK;
}

template <typename T>
static int loop_vjp_t(const LoopVjpArgs<T>& a, hipStream_t st) {
  return dispatch_nxnu(a.nx, a.nu, [&](auto cx, auto cu) {
    return dispatch_bs<4>(a.n, [&](auto bs) {
      return launch_loop_vjp<T, decltype(cx)::value, decltype(cu)::value, decltype(bs)::value>(
          a, st);
    });
  });
}

}  // namespace mpcqp

extern "C" int mpcqp_mpc_box_loop_vjp(int dtype, int batch, int nx, int nu, int N, int steps,
                                      const void* H, int64_t strideH, const void* F,
                                      int64_t strideF, const void* A, int64_t strideA,
                                      const void* Bm, int64_t strideB, const void* lb,
                                      int64_t strideLb, const void* ub, int64_t strideUb,
                                      const void* xs, const void* zs, const int32_t* status,
                                      const void* gxs, const void* gus, const void* gzs, void* gx0,
                                      void* gH, void* gF, void* gA, void* gB, void* glb, void* gub,
                                      void* gg, void* gw, int32_t* vstatus, void* stream) {
  using namespace mpcqp;
  const char* who = "mpcqp_mpc_box_loop_vjp";
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "%s: bad dtype %d", who, dtype);
  MPCQP_CHECK_ARG(batch >= 0 && N >= 1 && steps >= 0, "%s: bad sizes", who);
  MPCQP_CHECK_LOOP_SIZES(who, nx, nu, N);
  if (batch == 0) return MPCQP_OK;
  MPCQP_CHECK_ARG(H && F && A && Bm, "%s: H, F, A, B are required", who);
  MPCQP_CHECK_ARG(steps == 0 || (xs && zs), "%s: xs and zs are required for steps > 0", who);
  MPCQP_CHECK_ARG(strideH >= 0 && strideF >= 0 && strideA >= 0 && strideB >= 0 &&
                      strideLb >= 0 && strideUb >= 0,
                  "%s: negative stride", who);
  auto run = [&](auto tp) {
    using T = decltype(tp);
    LoopVjpArgs<T> a;
    a.batch = batch; a.nx = nx; a.nu = nu; a.n = N * nu; a.steps = steps;
    a.H = (const T*)H; a.sH = strideH; a.F = (const T*)F; a.sF = strideF;
    a.A = (const T*)A; a.sA = strideA; a.B = (const T*)Bm; a.sB = strideB;
    a.lb = (const T*)lb; a.slb = strideLb; a.ub = (const T*)ub; a.sub = strideUb;
    a.xs = (const T*)xs; a.zs = (const T*)zs; a.status = status;
    a.gxs = (const T*)gxs; a.gus = (const T*)gus; a.gzs = (const T*)gzs;
    a.gx0 = (T*)gx0; a.gH = (T*)gH; a.gF = (T*)gF; a.gA = (T*)gA; a.gB = (T*)gB;
    a.glb = (T*)glb; a.gub = (T*)gub; a.gg = (T*)gg; a.gw = (T*)gw; a.vstatus = vstatus;
    return loop_vjp_t<T>(a, (hipStream_t)stream);
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}
