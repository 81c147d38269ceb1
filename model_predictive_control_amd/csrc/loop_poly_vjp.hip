// loop_poly_vjp.hip -- mpcqp_mpc_poly_loop_vjp: the adjoint of the one-launch
// state-constrained MPC loop (loop_poly.hip, hard and affine), the whole
// reverse-time recursion in ONE launch, one instance per wavefront on the
// Sym2D register grid of the forward.
//
// Forward (mpcqp_mpc_poly_loop[_affine]), per instance, t = 0..T-1, C = [G; I]:
//     z_t = argmin 1/2 z'Hz + (F x_t + g_t)'z
//           s.t. hl - E x_t - e_t <= G z <= hu - E x_t - e_t,  lbz <= z <= ubz
//     u_t = z_t[0..nu),   x_{t+1} = A x_t + B u_t + w_t
// and y_t the signed multipliers, an exact 0 on every inactive row.  With the
// upstream gradients gxs, gus, gzs, gys (each may be absent = 0) and the shared
// factors of mpcqp_poly_setup (Hinv, Ut = C Hinv, M = C Hinv C', Kt = (-Hinv F)',
// L = -Ut F):
//     lam <- gxs[T]
//     for t = T-1 .. 0:
//         v    = gus[t] + B'lam;   gz = gzs[t], gz[0..nu) += v
//         A_t  = {i : y_t,i != 0}
//         r    = Ut gz,  q = Hinv gz
//         eps  = M_AA^-1 (r_A - gys[t]_A) on A_t, 0 elsewhere      geps[t]
//         gf[t] = -(q - Ut_A' eps_A),   gw[t] = lam
//         ghu += eps where y_t > 0,  ghl += eps where y_t < 0
//         lam <- gxs[t] + A'lam + Kt gz - (L + [E; 0])_A' eps_A
//     gx0 = lam
// eps, the Ut' eps tail of gf, Kt gz and the L' eps tail of lam are the code of
// poly_vjp_core.hpp, which poly_vjp_kernel calls too: on the same ys, gzs and
// gys a step's eps and gf are those of mpcqp_poly_solve_vjp bit for bit, and
// no round-off drifts over T.  Only v, and through it Ut[:, :nu] v,
// Hinv[:, :nu] v and Kt[:, :nu] v, depend on lam: the products with gzs[t] are
// hoisted.  -Hinv gzs[t] and -Ut gzs[t] of all steps are one prior launch of
// poly_affine_prep_kernel (poly_prep.hpp) over steps x batch rows into the
// caller's scratch; without gzs there is no such launch and no scratch.
// Kt gzs[t] is formed in the kernel, one step ahead.
//
// On chip for the episode: packed M, L + [E; 0] (row-major: the adjoint reads
// L' -- lane = state entry k, one active row r at a time -- so consecutive
// lanes read consecutive words, where the forward's transposed copy would put
// them NMAX words apart), A, B and the first nu columns of Ut and Kt in LDS;
// lam (lane k holds entry k), the ghl / ghu accumulators and diag M (one row
// per lane) in registers.  Per step W is reloaded from the LDS copy of M
// (poly_vjp_step).  The rows of step t-1 that do not depend on lam (ys, gys,
// -Ut gzs, gxs, gus, Kt gzs) are loaded before step t's sweeps, the
// one-step-ahead pattern of loop_box_vjp.hip.
//
// An instance whose outcome is not OPTIMAL gets exact zeros in every output,
// its rows of geps, gf and gw included (rewritten in the epilogue by the lanes
// that wrote them).  No atomics; every sum has a fixed order.
#include "poly_prep.hpp"
#include "poly_vjp_core.hpp"

#include "../../include/mpcqp_poly_loop_diff.h"

namespace mpcqp {

// every upstream gradient, status, E and every output but vstatus may be null
template <typename T>
struct PolyLoopVjpArgs : PolyFactors<T> {
  int batch, n, m, mt, nx, nu, steps;
  const T* E;                  // m x nx
  const T* A; const T* B;      // plant
  const T* ys;                 // steps x batch x mt
  const int32_t* status;       // steps x batch
  const T* gxs;                // (steps + 1) x batch x nx
  const T* gus;                // steps x batch x nu
  const T* gzs;                // steps x batch x n
  const T* gys;                // steps x batch x mt
  const T* nq;                 // -Hinv gzs, steps x batch x n   (null with gzs)
  const T* nr;                 // -Ut gzs,   steps x batch x mt  (null with gzs)
  T *gx0, *ghl, *ghu;          // batch x nx, batch x mt, batch x mt
  T *geps, *gf, *gw;           // steps x batch x mt, x n, x nx
  int32_t* vstatus;
};

// LDS elements: Sym2D scratch, the mat-vec partials, packed M, L + [E; 0]
// (NMAX x nx), A, B, the first nu columns of Ut (NMAX x nu) and Kt (nx x nu).
__host__ __device__ inline int poly_loop_vjp_lds(int BS, int mt, int nx, int nu) {
  const int NMAX = 8 * BS;
  return NMAX * BS + NMAX + 8 * NMAX + mt * (mt + 1) / 2 + nx * NMAX + nx * nx + nx * nu +
         NMAX * nu + nx * nu;
}

template <typename T, int BS>
__global__ __launch_bounds__(64) void poly_loop_vjp_kernel(PolyLoopVjpArgs<T> a) {
  using S2 = Sym2D<T, BS>;
  constexpr int NMAX = S2::NMAX;
  static_assert(NMAX <= kWave, "one row per lane");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int mt = a.mt, m = a.m, nz = a.n, nx = a.nx, nu = a.nu, steps = a.steps;
  const int P = mt * (mt + 1) / 2;
  T* buf = reinterpret_cast<T*>(smem_raw);
  T* part = buf + S2::BUF;
  T* Ps = part + 8 * NMAX;
  T* LEs = Ps + P;
  T* As = LEs + nx * NMAX;
  T* Bs = As + nx * nx;
  T* Un = Bs + nx * nu;
  T* Kn = Un + NMAX * nu;

  // ------------------------------------------------------------- stage in
  stage_packed<T, NMAX*(NMAX + 1) / 2>(a.M, Ps, P, lane);
  for (int e = lane; e < nx * NMAX; e += kWave) {
    const int r = e / nx;
    T v = r < mt ? a.L[e] : T(0);
    if (a.E && r < m) v += a.E[e];
    LEs[e] = v;
  }
  for (int e = lane; e < nx * nx; e += kWave) As[e] = a.A[e];
  for (int e = lane; e < nx * nu; e += kWave) {
    const int k = e / nu, j = e - k * nu;
    Bs[e] = a.B[e];
    Kn[e] = a.Kt[(int64_t)k * nz + j];
  }
  for (int e = lane; e < NMAX * nu; e += kWave) {
    const int r = e / nu, j = e - r * nu;
    Un[e] = r < mt ? a.Ut[(int64_t)r * nz + j] : T(0);
  }
  __syncthreads();

  const bool row = lane < mt;
  const int lr = lane < NMAX ? lane : 0;  // this lane's row of Un
  const int lk = lane < nx ? lane : 0;    // this lane's state entry
  const int lj = lane < nu ? lane : 0;    // this lane's input entry
  const T md = row ? Ps[lane * (lane + 1) / 2 + lane] : T(1);

  // The forward's own failure goes first: the code of the earliest step that
  // did not end OPTIMAL (it wrote NaN into y for every code but MAXITER, and
  // NONFINITE here would hide the cause).  A step of the soft loop that ended
  // with a slack solved another problem than the one differentiated here.
  int code0 = MPCQP_STATUS_OPTIMAL;
  if (a.status) {
    for (int base = 0; base < steps && code0 == MPCQP_STATUS_OPTIMAL; base += kWave) {
      const int t = base + lane;
      const int word = t < steps ? a.status[(int64_t)t * a.batch + b] : 0;
      int c = word & 0xff;
      if (c == MPCQP_STATUS_OPTIMAL && (word & MPCQP_STATUS_SOFTENED)) c = MPCQP_STATUS_INFEASIBLE;
      const uint64_t bad = __builtin_amdgcn_ballot_w64(c != MPCQP_STATUS_OPTIMAL);
      if (bad) code0 = readlane(c, uniform(__builtin_ctzll(bad)));
    }
  }
  if (code0 == MPCQP_STATUS_OPTIMAL && *a.flag) code0 = MPCQP_STATUS_NOT_CONVEX;
  code0 = uniform(code0);

  // lam = gxs[T]: lane k holds entry k
  T lam = (a.gxs && lane < nx) ? a.gxs[((int64_t)steps * a.batch + b) * nx + lane] : T(0);
  bool nonfin = __any(!finite(lam));
  bool notconv = false;
  T accl = T(0), accu = T(0);  // ghl, ghu of row `lane`

  // This lane's entries of a step's rows that do not depend on lam, loaded one
  // step ahead: row `lane` of ys[t], gys[t] and -Ut gzs[t], entry `lane` of
  // gxs[t], gus[t] and Kt gzs[t]; 0 where there is none.
  T yn = T(0), gyn = T(0), rn = T(0), sn = T(0), un = T(0), kn = T(0);
  bool nfn = false;  // a NaN/Inf in gzs[t] or -Hinv gzs[t]
  auto fetch = [&](int t) {
    const int64_t rb = (int64_t)t * a.batch + b;
    if (row) {
      yn = a.ys[rb * mt + lane];
      if (a.gys) gyn = a.gys[rb * mt + lane];
      if (a.nr) rn = a.nr[rb * mt + lane];
    }
    if (a.gxs && lane < nx) sn = a.gxs[rb * nx + lane];
    if (a.gus && lane < nu) un = a.gus[rb * nu + lane];
    if (a.gzs) {
      const T* gz = a.gzs + rb * nz;
      nfn = false;
      for (int j = lane; j < nz; j += kWave) nfn |= !finite(gz[j]) || !finite(a.nq[rb * nz + j]);
      kn = kt_gz(a.Kt, gz, nz, nx, lane);
    }
  };
  const bool go = code0 == MPCQP_STATUS_OPTIMAL;
  if (go && steps > 0) fetch(steps - 1);

  S2 W;
  W.init(lane);

  for (int t = go ? steps - 1 : -1; t >= 0; --t) {
    const int64_t rb = (int64_t)t * a.batch + b;
    const T yi = yn, gyi = gyn, sx = sn, kg = kn;
    nonfin = nonfin || __any(!finite(yi) || !finite(gyi) || !finite(rn) || !finite(sx) ||
                             !finite(un) || !finite(kg) || nfn);
    // v = gus[t] + B'lam (lane j holds entry j); r = Ut gzs[t] + Ut[:, :nu] v
    T v = un;
    for (int k = 0; k < nx; ++k) v = fma(Bs[k * nu + lj], readlane(lam, k), v);
    T ri = -rn;
    for (int j = 0; j < nu; ++j) ri = fma(Un[lr * nu + j], readlane(v, j), ri);
    // the rows of step t - 1: in flight during the sweeps below
    if (t > 0) fetch(t - 1);

    const bool run = !nonfin && !notconv;
    bool ok = run;
    uint64_t emask = 0;
    T ei = T(0);
    if (run) {
      bool unused = false;  // a NaN/Inf in M is not reported as such here
      W.load_packed(Ps, mt, unused);
      ei = poly_vjp_step<T, BS>(W, buf, part, md, row && yi != T(0), ri - gyi, ok, emask);
      notconv = !ok;
    }
    if (row) {
      if (a.geps) a.geps[rb * mt + lane] = ei;
      accl += yi < T(0) ? ei : T(0);
      accu += yi > T(0) ? ei : T(0);
    }
    if (a.gw && lane < nx) a.gw[rb * nx + lane] = lam;
    // gf_j = -q_j + sum over A of Ut[r][j] eps_r,  -q = -Hinv gzs[t] - Hinv[:, :nu] v
    // (Hinv is symmetric: its rows are read along j)
    if (a.gf && ok) {
      for (int j = lane; j < nz; j += kWave) {
        T acc = a.nq ? a.nq[rb * nz + j] : T(0);
        for (int i = 0; i < nu; ++i) acc = fma(-a.Hinv[(int64_t)i * nz + j], readlane(v, i), acc);
        a.gf[rb * nz + j] = gf_tail(a.Ut, nz, j, ei, emask, acc);
      }
    }
    // lam <- gxs[t] + A'lam + Kt gzs[t] + Kt[:, :nu] v - (L + [E; 0])_A' eps_A
    T ln = kg;
    for (int j = 0; j < nu; ++j) ln = fma(Kn[lk * nu + j], readlane(v, j), ln);
    ln = lt_e_tail(LEs, nx, lk, ei, emask, ln);
    for (int i = 0; i < nx; ++i) ln = fma(As[i * nx + lk], readlane(lam, i), ln);
    lam = lane < nx ? ln + sx : T(0);
  }

  // ------------------------------------------------------------- epilogue
  int code = code0;
  if (code == MPCQP_STATUS_OPTIMAL && nonfin) code = MPCQP_STATUS_NONFINITE;
  if (code == MPCQP_STATUS_OPTIMAL && notconv) code = MPCQP_STATUS_NOT_CONVEX;
  const bool ok = code == MPCQP_STATUS_OPTIMAL;
  if (lane == 0) a.vstatus[b] = code;
  if (row) {
    if (a.ghl) a.ghl[(int64_t)b * mt + lane] = ok ? accl : T(0);
    if (a.ghu) a.ghu[(int64_t)b * mt + lane] = ok ? accu : T(0);
  }
  if (a.gx0 && lane < nx) a.gx0[(int64_t)b * nx + lane] = ok ? lam : T(0);
  // A failure zeroes the rows of geps, gf and gw: a failed forward left them
  // unwritten, a failure found mid-episode leaves the rows of the later steps
  // behind.  The lanes that wrote an entry rewrite it, so the two stores to an
  // address are one lane's, in program order.
  if (!ok) {
    for (int t = 0; t < steps; ++t) {
      const int64_t rb = (int64_t)t * a.batch + b;
      if (a.geps && row) a.geps[rb * mt + lane] = T(0);
      if (a.gw && lane < nx) a.gw[rb * nx + lane] = T(0);
      if (a.gf)
        for (int j = lane; j < nz; j += kWave) a.gf[rb * nz + j] = T(0);
    }
  }
}

template <typename T, int BS>
static int launch_poly_loop_vjp(const PolyLoopVjpArgs<T>& a, hipStream_t st) {
  const size_t bytes = (size_t)poly_loop_vjp_lds(BS, a.mt, a.nx, a.nu) * sizeof(T);
  if (bytes > 64 * 1024) {
    set_error("mpcqp_mpc_poly_loop_vjp: %zu B of LDS needed, 65536 available", bytes);
    return MPCQP_ENOTSUP;
  }
  hipLaunchKernelGGL((poly_loop_vjp_kernel<T, BS>), dim3((unsigned)a.batch), dim3(kWave), bytes,
                     st, a);
  MPCQP_CHECK_LAUNCH("poly_loop_vjp_kernel");
  return MPCQP_OK;
}

}  // namespace mpcqp

extern "C" size_t mpcqp_mpc_poly_loop_vjp_workspace(int dtype, int batch, int n, int m, int nbox,
                                                    int steps) {
  const int mt = m + (nbox ? n : 0);
  if (!mpcqp::poly_vjp_sizes_ok(dtype, n, m, mt) || batch < 0 || steps < 0) return 0;
  return (size_t)mpcqp::poly_vjp_ws(mpcqp::dtype_size(dtype), (int64_t)steps * batch, n, mt).total;
}

// The argument checks, all before any device work.
extern "C" int mpcqp_mpc_poly_loop_vjp(int dtype, int batch, int n, int m, int nbox, int nx, int nu,
                                       int steps, const void* workspace, const void* E,
                                       const void* A, const void* Bm, const void* ys,
                                       const int32_t* status, const void* gxs, const void* gus,
                                       const void* gzs, const void* gys, void* gx0, void* ghl,
                                       void* ghu, void* geps, void* gf, void* gw, int32_t* vstatus,
                                       void* scratch, size_t scratch_bytes, void* stream) {
  using namespace mpcqp;
  const char* who = "mpcqp_mpc_poly_loop_vjp";
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "%s: bad dtype %d", who, dtype);
  MPCQP_CHECK_ARG(batch >= 0 && n >= 1 && m >= 0 && steps >= 0,
                  "%s: bad sizes batch=%d n=%d m=%d steps=%d", who, batch, n, m, steps);
  const int mt = m + (nbox ? n : 0);
  MPCQP_CHECK_ARG(mt >= 1 && mt <= 64, "%s: rows m_total=%d outside [1,64]", who, mt);
  MPCQP_CHECK_ARG(nx >= 1 && nx <= 16 && nu >= 1 && nu <= 16 && nu <= n,
                  "%s: nx=%d nu=%d outside 1 <= nx <= 16, 1 <= nu <= min(16, n)", who, nx, nu);
  if (batch == 0) return MPCQP_OK;
  MPCQP_CHECK_ARG(workspace && A && Bm && vstatus, "%s: workspace, A, B and vstatus are required",
                  who);
  MPCQP_CHECK_ARG(steps == 0 || ys, "%s: ys is required for steps > 0", who);
  const int64_t rows = (int64_t)steps * batch;
  const PolyVjpWs S = poly_vjp_ws(dtype_size(dtype), rows, n, mt);
  const bool prep = gzs && steps > 0;
  MPCQP_CHECK_ARG(!prep || (scratch && scratch_bytes >= (size_t)S.total),
                  "%s: gzs needs %lld B of scratch, %zu given", who, (long long)S.total,
                  scratch ? scratch_bytes : (size_t)0);
  hipStream_t st = (hipStream_t)stream;
  const PolyWs L = poly_ws(dtype_size(dtype), n, mt, nx);
  const char* base = (const char*)workspace;
  if (prep) {
    const int rc = launch_poly_affine_prep(who, dtype, gzs, rows, n, mt, base + L.oHinv,
                                           base + L.oUt, (char*)scratch + S.oQ,
                                           (char*)scratch + S.oR, st);
    if (rc != MPCQP_OK) return rc;
  }
  auto run = [&](auto tp) {
    using T = decltype(tp);
    PolyLoopVjpArgs<T> a;
    set_poly_factors<T>(a, workspace, L);
    a.batch = batch; a.n = n; a.m = m; a.mt = mt; a.nx = nx; a.nu = nu; a.steps = steps;
    a.E = m > 0 ? (const T*)E : nullptr; a.A = (const T*)A; a.B = (const T*)Bm;
    a.ys = (const T*)ys; a.status = status;
    a.gxs = (const T*)gxs; a.gus = (const T*)gus; a.gys = (const T*)gys;
    a.gzs = prep ? (const T*)gzs : nullptr;
    a.nq = prep ? (const T*)((const char*)scratch + S.oQ) : nullptr;
    a.nr = prep ? (const T*)((const char*)scratch + S.oR) : nullptr;
    a.gx0 = (T*)gx0; a.ghl = (T*)ghl; a.ghu = (T*)ghu;
    a.geps = (T*)geps; a.gf = (T*)gf; a.gw = (T*)gw;
    a.vstatus = vstatus;
    return dispatch_bs<8>(mt, [&](auto bs) {
      return launch_poly_loop_vjp<T, decltype(bs)::value>(a, st);
    });
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}
