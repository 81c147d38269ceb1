// poly_vjp.hip -- the adjoint of the stand-alone polytope QP
// (mpcqp_poly_solve_vjp, include/mpcqp_poly_diff.h), one instance per
// wavefront on the Sym2D register grid of the forward (solve_poly.hip).  The
// algebra and the step itself are in poly_vjp_core.hpp; here are the two
// launches, the staging and the status rules.
//   1. q and r of every instance: the skinny GEMM poly_affine_prep_kernel of
//      loop_poly.hip (poly_prep.hpp), which writes -Hinv gz and -Ut gz into the
//      caller's scratch; an element of Hinv / Ut is loaded once per 16
//      instances, not once per instance.
//   2. poly_vjp_kernel: M staged as the forward does, one poly_vjp_step, then
//      ghu_i = e_i (y_i > 0), ghl_i = e_i (y_i < 0), gf = -q + Ut_A' e_A over
//      lanes strided by 64 in j, gx0 = Kt gz - L_A' e_A.
// vstatus: the forward's code if that is not OPTIMAL, else NOT_CONVEX (H not
// positive definite), NONFINITE (an input or M), NOT_CONVEX (the rows marked
// active are dependent).  An instance whose vstatus is not OPTIMAL gets exact
// zeros in every output (a NaN would poison the batch sum of a shared
// operand's gradient).  No atomics; every sum has a fixed order.
#include "poly_prep.hpp"
#include "poly_vjp_core.hpp"

#include "../../include/mpcqp_poly_diff.h"

namespace mpcqp {

// status, gz (with nq, nr), gy and every output may be null
template <typename T>
struct PolyVjpArgs : PolyFactors<T> {
  int batch, n, mt, nx;        // nx = 0 without gx0
  const T* y;
  const int32_t* status;
  const T* gz;
  const T* gy;
  const T* nq;                 // -Hinv gz, batch x n   (null with gz)
  const T* nr;                 // -Ut gz,   batch x mt  (null with gz)
  T *gf, *gx0, *ghl, *ghu;
  int32_t* vstatus;
};

template <typename T, int BS>
__global__ __launch_bounds__(64) void poly_vjp_kernel(PolyVjpArgs<T> a) {
  using S2 = Sym2D<T, BS>;
  constexpr int NMAX = S2::NMAX;
  static_assert(NMAX <= kWave, "one row per lane");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* buf = reinterpret_cast<T*>(smem_raw);
  T* part = buf + S2::BUF;     // 8 * NMAX: partial row sums of the mat-vec
  T* Ps = part + 8 * NMAX;
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int mt = a.mt;
  const int P = mt * (mt + 1) / 2;
  const int nz = a.n, nx = a.nx;
  stage_packed<T, NMAX*(NMAX + 1) / 2>(a.M, Ps, P, lane);
  __syncthreads();
  // row `lane`: y, gy, r = Ut gz and M_ii
  const bool row = lane < mt;
  T yi = T(0), gyi = T(0), ri = T(0), md = T(1);
  if (row) {
    const int64_t o = (int64_t)b * mt + lane;
    yi = a.y[o];
    if (a.gy) gyi = a.gy[o];
    if (a.nr) ri = -a.nr[o];
    md = Ps[lane * (lane + 1) / 2 + lane];
  }
  bool nonfinite = row && (!finite(yi) || !finite(gyi) || !finite(ri));
  for (int j = lane; j < nz; j += kWave) {
    const int64_t o = (int64_t)b * nz + j;
    const T gzj = a.gz ? a.gz[o] : T(0);
    const T qj = a.nq ? a.nq[o] : T(0);
    nonfinite |= !finite(gzj) || !finite(qj);
  }
  S2 W;
  W.init(lane);
  W.load_packed(Ps, mt, nonfinite);  // a NaN/Inf in M counts as NONFINITE here

  // The forward's own failure goes first: it wrote NaN into y and z, and
  // NONFINITE here would hide the cause.
  int code = a.status ? (a.status[b] & 0xff) : MPCQP_STATUS_OPTIMAL;
  if (code == MPCQP_STATUS_OPTIMAL) {
    if (*a.flag) code = MPCQP_STATUS_NOT_CONVEX;
    else if (__any(nonfinite)) code = MPCQP_STATUS_NONFINITE;
  }
  code = uniform(code);
  const bool act = code == MPCQP_STATUS_OPTIMAL && row && yi != T(0);
  bool swept;
  uint64_t emask;
  const T ei = poly_vjp_step<T, BS>(W, buf, part, md, act, ri - gyi, swept, emask);
  if (!swept) code = MPCQP_STATUS_NOT_CONVEX;
  const bool ok = code == MPCQP_STATUS_OPTIMAL;
  if (row) {
    const int64_t o = (int64_t)b * mt + lane;
    if (a.ghl) a.ghl[o] = yi < T(0) ? ei : T(0);
    if (a.ghu) a.ghu[o] = yi > T(0) ? ei : T(0);
  }
  // gf_j = -q_j + sum over A of Ut[r][j] e_r   (lanes over j, coalesced rows)
  if (a.gf) {
    for (int j = lane; j < nz; j += kWave) {
      const int64_t o = (int64_t)b * nz + j;
      const T qj = a.nq ? -a.nq[o] : T(0);
      const T acc = gf_tail(a.Ut, nz, j, ei, emask, -qj);
      a.gf[o] = ok ? acc : T(0);
    }
  }
  // gx0_k = sum_j Kt[k][j] gz_j - sum over A of L[r][k] e_r
  if (a.gx0) {
    T gk = kt_gz(a.Kt, a.gz ? a.gz + (int64_t)b * nz : nullptr, nz, nx, lane);
    if (lane < nx) {
      gk = lt_e_tail(a.L, nx, lane, ei, emask, gk);
      a.gx0[(int64_t)b * nx + lane] = ok ? gk : T(0);
    }
  }
  if (lane == 0) a.vstatus[b] = code;
}

template <typename T, int BS>
static int launch_poly_vjp(const PolyVjpArgs<T>& a, hipStream_t st) {
  const size_t bytes =
      (size_t)(Sym2D<T, BS>::BUF + 8 * Sym2D<T, BS>::NMAX + a.mt * (a.mt + 1) / 2) * sizeof(T);
  hipLaunchKernelGGL((poly_vjp_kernel<T, BS>), dim3((unsigned)a.batch), dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("poly_vjp_kernel");
  return MPCQP_OK;
}

}  // namespace mpcqp

extern "C" size_t mpcqp_poly_solve_vjp_workspace(int dtype, int batch, int n, int m, int nbox) {
  const int mt = m + (nbox ? n : 0);
  if (!mpcqp::poly_vjp_sizes_ok(dtype, n, m, mt) || batch <= 0) return 0;
  return (size_t)mpcqp::poly_vjp_ws(mpcqp::dtype_size(dtype), batch, n, mt).total;
}

// The argument checks, all before any device work.
extern "C" int mpcqp_poly_solve_vjp(int dtype, int batch, int n, int m, int nbox, int nx,
                                    const void* workspace, const void* y, const int32_t* status,
                                    const void* gz, const void* gy, void* gf, void* gx0,
                                    void* ghl, void* ghu, int32_t* vstatus, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  using namespace mpcqp;
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "mpcqp_poly_solve_vjp: bad dtype %d",
                  dtype);
  MPCQP_CHECK_ARG(n >= 1 && m >= 0 && nx >= 0 && nx <= 16,
                  "mpcqp_poly_solve_vjp: bad sizes n=%d m=%d nx=%d (n >= 1, m >= 0, 0 <= nx <= 16)",
                  n, m, nx);
  const int mt = m + (nbox ? n : 0);
  MPCQP_CHECK_ARG(mt >= 1 && mt <= 64, "mpcqp_poly_solve_vjp: rows m_total=%d outside [1,64]", mt);
  MPCQP_CHECK_ARG(batch >= 0, "mpcqp_poly_solve_vjp: batch < 0");
  MPCQP_CHECK_ARG(gx0 == nullptr || nx > 0, "mpcqp_poly_solve_vjp: gx0 given but nx = 0");
  if (batch == 0) return MPCQP_OK;
  MPCQP_CHECK_ARG(workspace && y && vstatus,
                  "mpcqp_poly_solve_vjp: workspace, y and vstatus are required");
  const PolyVjpWs S = poly_vjp_ws(dtype_size(dtype), batch, n, mt);
  MPCQP_CHECK_ARG(!gz || (scratch && scratch_bytes >= (size_t)S.total),
                  "mpcqp_poly_solve_vjp: gz needs %lld B of scratch, %zu given",
                  (long long)S.total, scratch ? scratch_bytes : (size_t)0);
  hipStream_t st = (hipStream_t)stream;
  const PolyWs L = poly_ws(dtype_size(dtype), n, mt, nx);
  const char* base = (const char*)workspace;
  if (gz) {
    const int rc = launch_poly_affine_prep("mpcqp_poly_solve_vjp", dtype, gz, batch, n, mt,
                                           base + L.oHinv, base + L.oUt, (char*)scratch + S.oQ,
                                           (char*)scratch + S.oR, st);
    if (rc != MPCQP_OK) return rc;
  }
  auto run = [&](auto tp) {
    using T = decltype(tp);
    PolyVjpArgs<T> a;
    set_poly_factors<T>(a, workspace, L);
    a.batch = batch; a.n = n; a.mt = mt; a.nx = gx0 ? nx : 0;
    a.y = (const T*)y; a.status = status;
    a.gz = (const T*)gz; a.gy = (const T*)gy;
    a.nq = gz ? (const T*)((const char*)scratch + S.oQ) : nullptr;
    a.nr = gz ? (const T*)((const char*)scratch + S.oR) : nullptr;
    a.gf = (T*)gf; a.gx0 = (T*)gx0; a.ghl = (T*)ghl; a.ghu = (T*)ghu;
    a.vstatus = vstatus;
    return dispatch_bs<8>(mt, [&](auto bs) {
      return launch_poly_vjp<T, decltype(bs)::value>(a, st);
    });
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}
