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
// The four groups of a wave hold different free sets: the sweep loop runs
// while any group has a row left, every group passes every LDS publish of
// QSym::column, and a group with nothing left to sweep discards what it read
// (the "H swept on the guessed free rows only" loop of loop_box.hip).
//
// A row at a bound with a zero multiplier counts as active: the result is the
// one-sided derivative on the side that keeps it there.  An instance whose
// outcome is not OPTIMAL gets exact zeros in every gradient (a NaN would
// poison the batch sum of a shared parameter's gradient); the caller has
// vstatus.  Division is IEEE: the pivot reciprocal is a plain division
// (sweep_col_ieee, sweep_ieee.hpp) and the file is built without the
// approximate-division flags.
#include "quad_api.hpp"
#include "sweep_ieee.hpp"

namespace mpcqp {

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

  // rows bi*BS + r of this lane: z, g and the row's state
  // (0 free, 1 at lb, 2 at ub, 3 past n); lb == ub == z counts as "at lb"
  T zr[BS], gr[BS];
  int st[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    const int i = M.bi * BS + r;
    zr[r] = zs[i];
    gr[r] = gzs[i];
    st[r] = i < n ? (zr[r] == lbs[i] ? 1 : (zr[r] == ubs[i] ? 2 : 0)) : 3;
  }
  // free-row mask of the group (rows bi*BS + r from the bj == 0 lanes)
  unsigned fmask = 0;
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    const unsigned long long bal = __ballot(M.bj == 0 && st[r] == 0);
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
      if ((bal >> (16 * g + 4 * bb)) & 1ull) fmask |= 1u << (bb * BS + r);
  }
  if (!run) fmask = 0;
  // ---------------------------------------- M = SWEEP_F(H), wave-uniform trips
  bool okp = true;
  while (__any(fmask != 0)) {
    const bool has = fmask != 0;
    const int k = has ? __builtin_ctz(fmask) : 0;
    fmask = has ? fmask & (fmask - 1) : 0u;
    T colr[BS], colc[BS];
    const T d = M.column(k, gb, colr, colc);
    if (has) {
      okp = okp && d > T(0);
      sweep_col_ieee(M, k, d, colr, colc);
    }
  }
  if (code == MPCQP_STATUS_OPTIMAL && !okp) code = MPCQP_STATUS_NOT_CONVEX;
  const bool good = live && code == MPCQP_STATUS_OPTIMAL;
  // ------------------------------------------------------ out = M [g_F; 0]
  T w[BS], out[BS], dr[BS], nur[BS];
#pragma unroll
  for (int r = 0; r < BS; ++r) w[r] = (good && st[r] == 0) ? gr[r] : T(0);
  M.matvec(w, gb, out);
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    dr[r] = (good && st[r] == 0) ? out[r] : T(0);
    nur[r] = (good && (st[r] == 1 || st[r] == 2)) ? gr[r] - out[r] : T(0);
  }
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
            Ps[i * (i + 1) / 2 + j] = good ? v : T(0);
          }
        }
    }
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

template <typename T>
int solve_box_vjp_quad(const BoxVjpArgs<T>& a, hipStream_t st) {
  return dispatch_bs<4>(a.n, [&](auto bs) {
    return launch_box_vjp<T, decltype(bs)::value>(a, st);
  });
}

template int solve_box_vjp_quad<double>(const BoxVjpArgs<double>&, hipStream_t);
template int solve_box_vjp_quad<float>(const BoxVjpArgs<float>&, hipStream_t);

}  // namespace mpcqp
