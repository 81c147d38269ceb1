// box_vjp.hip -- the adjoint of the box QP for n <= 32 (mpcqp_solve_box_vjp),
// FOUR instances per wavefront on the QSym layout of quad.hpp, one per 16-lane
// DPP row, as box_quad_kernel (quad_box.hip) runs the forward solve.
//
// At the optimum z of  min 1/2 z'Hz + f'z, lb <= z <= ub  let A be the rows
// held at a bound (z_i == lb_i or z_i == ub_i, compared exactly: the active
// set writes active rows as the bound itself) and F the free rows.  With
// g = dL/dz:
//     d_F  = -H_FF^{-1} g_F,   d_A = 0             dL/df = d
//     nu_A = g_A + H_AF d_F,   nu_F = 0            dL/dlb_i = nu_i at lb_i,
//                                                  dL/dub_i = nu_i at ub_i
//     dL/dH (full, unsymmetrised) = d z'           packed (i, j<i): d_i z_j + d_j z_i
//                                                  packed (i, i):   d_i z_i
// H swept on the free rows only, M = SWEEP_F(H), has M_FF = -H_FF^{-1} and
// M_AF = H_AF H_FF^{-1}, so one mat-vec out = M [g_F; 0] yields d_F = out_F and
// nu_A = g_A - out_A: |F| sweeps and one product, no iterations.
//
// The step itself (row states, sweeps, product, d and nu) and the fold of d z'
// are box_vjp_core.hpp, shared with loop_box_vjp.hip.
//
// A row at a bound with a zero multiplier counts as active: the result is the
// one-sided derivative on the side that keeps it there.  An instance whose
// outcome is not OPTIMAL gets exact zeros in every gradient (a NaN would
// poison the batch sum of a shared parameter's gradient); the caller has
// vstatus.  Division is IEEE: the pivot reciprocal is a plain division
// (sweep_col_ieee) and the file is built without the approximate-division
// flags.
#include "box_vjp_core.hpp"
#include "quad_api.hpp"

namespace mpcqp {

constexpr int kBoxVjpMaxN = 32;

// every output and status / vstatus may be null
template <typename T>
struct BoxVjpArgs {
  int batch, n;
  const T* H; int64_t sH;
  const T* z;
  const T* lb; int64_t slb;
  const T* ub; int64_t sub;
  const int32_t* status;
  const T* gz;
  T *gf, *glb, *gub, *gH;
  int32_t* vstatus;
};

// Per-group LDS: the QSym exchange tile, the row vectors z, lb, ub, g and d,
// and the packed tile (H on the way in, dL/dH on the way out).
template <typename T, int BS>
struct VjpLds {
  static constexpr int NMAX = QSym<T, BS>::NMAX;
  static constexpr int PMAX = NMAX * (NMAX + 1) / 2;
  static constexpr int oBuf = 0;
  static constexpr int oZ = QSym<T, BS>::BUF;
  static constexpr int oLb = oZ + NMAX;
  static constexpr int oUb = oLb + NMAX;
  static constexpr int oG = oUb + NMAX;
  static constexpr int oD = oG + NMAX;
  static constexpr int oP = oD + NMAX;
  static constexpr int size = (oP + PMAX + 1) & ~1;
};

template <typename T, int BS>
__global__ __launch_bounds__(64) void box_vjp_quad_kernel(BoxVjpArgs<T> a) {
  using L = VjpLds<T, BS>;
  constexpr int NMAX = L::NMAX;
  constexpr int PMAX = L::PMAX;
  constexpr int MAXT = (PMAX + 15) / 16;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int lane = threadIdx.x, g = lane >> 4, q = lane & 15;
  const int b = blockIdx.x * 4 + g;
  const bool live = b < a.batch;
  const int bl = live ? b : 0;
  const int n = a.n, P = n * (n + 1) / 2;
  T* gs = reinterpret_cast<T*>(smem_raw) + g * L::size;
  T* gb = gs + L::oBuf;
  T* zs = gs + L::oZ;
  T* lbs = gs + L::oLb;
  T* ubs = gs + L::oUb;
  T* gzs = gs + L::oG;
  T* ds = gs + L::oD;
  T* Ps = gs + L::oP;
  // ------------------------------------------------------------- stage in
  {
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
  const int fcode = (live && a.status) ? (a.status[b] & 0xff) : MPCQP_STATUS_OPTIMAL;
  bool nonfinite = false;
  for (int i = q; i < NMAX; i += 16) {
    const bool v = live && i < n;
    const T zi = v ? a.z[(int64_t)b * n + i] : T(0);
    const T gi = v ? a.gz[(int64_t)b * n + i] : T(0);
    const T li = (v && a.lb) ? a.lb[(int64_t)b * a.slb + i] : -Lim<T>::inf();
    const T ui = (v && a.ub) ? a.ub[(int64_t)b * a.sub + i] : Lim<T>::inf();
    zs[i] = zi;
    gzs[i] = gi;
    lbs[i] = li;
    ubs[i] = ui;
    nonfinite |= v && (!finite(zi) || !finite(gi));
  }
  __syncthreads();
  QSym<T, BS> M;
  M.init(lane);
  M.load_packed(Ps, n, nonfinite);
  const unsigned long long gmask = 0xFFFFull << (16 * g);
  const bool g_nonfinite = (__ballot(nonfinite) & gmask) != 0;
  // The forward's own failure goes first: it wrote NaN into z for every code
  // but MAXITER, and NONFINITE here would hide the cause.
  int code = fcode;
  if (code == MPCQP_STATUS_OPTIMAL && g_nonfinite) code = MPCQP_STATUS_NONFINITE;
  const bool run = live && code == MPCQP_STATUS_OPTIMAL;

  // ------------------------------------- the step (box_vjp_core.hpp): d and nu
  T zr[BS], dr[BS], nur[BS];
  int st[BS];
  const bool good = box_vjp_step(M, gb, zs, gzs, lbs, ubs, n, g, run, zr, st, dr, nur);
  if (run && !good) code = MPCQP_STATUS_NOT_CONVEX;
  if (live && M.bj == 0) {
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      const int i = M.bi * BS + r;
      if (i < n) {
        const int64_t o = (int64_t)b * n + i;
        if (a.gf) a.gf[o] = dr[r];
        if (a.glb) a.glb[o] = st[r] == 1 ? nur[r] : T(0);
        if (a.gub) a.gub[o] = st[r] == 2 ? nur[r] : T(0);
      }
    }
  }
  if (live && q == 0 && a.vstatus) a.vstatus[b] = code;
  // ----------------------------------------------- dL/dH = d z' (packed lower)
  // The block owners on and below the diagonal put their entries into the
  // packed tile; the group then stores the tile as it loaded H.
  if (a.gH) {
    if (M.bj == 0) {
#pragma unroll
      for (int r = 0; r < BS; ++r) ds[M.bi * BS + r] = dr[r];
    }
    lds_exchange();
    fold_dz(M, ds, zs, dr, zr, n, [&](int e, T v) { Ps[e] = good ? v : T(0); });
    lds_exchange();
    if (live) {
      T* Gb = a.gH + (int64_t)b * P;
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        const int e = q + 16 * t;
        if (e < P) Gb[e] = Ps[e];
      }
    }
  }
}

template <typename T, int BS>
static int launch_box_vjp(const BoxVjpArgs<T>& a, hipStream_t st) {
  const size_t bytes = (size_t)4 * VjpLds<T, BS>::size * sizeof(T);
  hipLaunchKernelGGL((box_vjp_quad_kernel<T, BS>), dim3((a.batch + 3) / 4), dim3(kWave), bytes, st,
                     a);
  MPCQP_CHECK_LAUNCH("box_vjp_quad_kernel");
  return MPCQP_OK;
}

}  // namespace mpcqp

// The argument checks, all before any device work.
extern "C" int mpcqp_solve_box_vjp(int dtype, int batch, int n, const void* H, int64_t strideH,
                                   const void* z, const void* lb, int64_t strideLb, const void* ub,
                                   int64_t strideUb, const int32_t* status, const void* gz,
                                   void* gf, void* glb, void* gub, void* gH, int32_t* vstatus,
                                   void* stream) {
  using namespace mpcqp;
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "mpcqp_solve_box_vjp: bad dtype %d",
                  dtype);
  MPCQP_CHECK_ARG(batch >= 0, "mpcqp_solve_box_vjp: batch < 0");
  MPCQP_CHECK_ARG(n >= 1, "mpcqp_solve_box_vjp: n=%d < 1", n);
  if (n > kBoxVjpMaxN) {
    set_error("mpcqp_solve_box_vjp: n=%d above the limit %d", n, kBoxVjpMaxN);
    return MPCQP_ENOTSUP;
  }
  if (batch == 0) return MPCQP_OK;
  MPCQP_CHECK_ARG(H && z && gz, "mpcqp_solve_box_vjp: H, z, gz are required");
  MPCQP_CHECK_ARG(strideH >= 0 && strideLb >= 0 && strideUb >= 0,
                  "mpcqp_solve_box_vjp: negative stride");
  auto run = [&](auto tp) {
    using T = decltype(tp);
    const BoxVjpArgs<T> a{batch, n, (const T*)H, strideH, (const T*)z, (const T*)lb, strideLb,
                          (const T*)ub, strideUb, status, (const T*)gz, (T*)gf, (T*)glb, (T*)gub,
                          (T*)gH, vstatus};
    return dispatch_bs<4>(n, [&](auto bs) {
      return launch_box_vjp<T, decltype(bs)::value>(a, (hipStream_t)stream);
    });
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}
