// loop_poly.hip -- mpcqp_mpc_poly_loop: the receding-horizon loop of a linear
// MPC with row (state) constraints and an input box, T steps in ONE launch, one
// instance per wavefront.
//
// Reference: the MPC of sessions 2 and 3 (session_2/problem.py:4-33: a double
// integrator with p_max, v_min, v_max and an input box; the per-step
// ControllerLog of session_2/log.py:8-12, whose solver_success is the status
// word here) run in closed loop on a linear plant (LinearSystem.py:20-26;
// simulate(...) main.py:270-271), with the state box in condensed form as
// rows of Gam with bounds shifted by the free response (main.py:58-61).  Per
// step t and instance b:
//   z_t = argmin 1/2 z'Hz + (F x_t)'z   s.t.  hl - E x_t <= G z <= hu - E x_t,
//                                              lbz <= z <= ubz
//   u_t = z_t[0..nu-1],   x_{t+1} = A x_t + B u_t (+ w_t)
//
// The QP is solved through its dual as in solve_poly.hip (dual range active
// set on W = SWEEP_A(M), register-resident on the Sym2D grid), on the shared
// factors of mpcqp_poly_setup.  Everything a step needs stays on chip for the
// whole episode: packed M, L, E, the plant and the first nu columns of Ut and
// Kt in LDS, W and the row states in registers.  Per step the HBM traffic is
// x, u, the status word and the optional w / zs / ys.
//
// Warm start: W and the row states st carry over, unshifted.  At the top of a
// step y is recomputed for the new s0 and bounds; while an active row's
// multiplier has the wrong sign for its side, the most wrong row is dropped
// (a reverse sweep) -- at most |A| drops, after which (z(A), y) is a
// dual-feasible pair and the ordinary iteration continues from it.
//
// Drift: W is reloaded from the LDS copy of M whenever a step ends with an
// empty active set, and rebuilt (reload, then the active rows swept back in)
// every kPolyLoopRebuild steps.
//
// The step is one loop with ONE sweep site (rebuild adds, repair drops and the
// iteration's adds and drops all pass through it), so that W lives in a single
// register set, as in dual_range_kernel.  Every trip counts against max_iter,
// except the rebuild sweeps, which a bit mask of at most mt rows bounds; every
// exit test is written so that a NaN operand ends the loop.
//
// mpcqp_mpc_poly_loop_soft is the SOFT instantiation of the same kernel: rows
// with an exact penalty on a shared slack instead of a hard bound, as a third
// row state inside the same active set (see poly_loop_kernel).
// The hard instantiation compiles to what it was without the variant.
//
// mpcqp_mpc_poly_loop_affine is the AFFINE instantiation (hard or soft): a
// per-step linear term g_t in the gradient and a shift e_t of the row bounds,
// both independent of the state, so that -Hinv g and -Ut g are formed for all
// steps at once by poly_affine_prep_kernel before the loop and the loop only
// adds them.  AFFINE is a template flag like SOFT: the four
// instantiations without it compile to what they were.
#include "dual_range_core.hpp"
#include "poly_prep.hpp"
#include "poly_ws.hpp"

// Steps between two rebuilds of W from M ("Poly loop").
#ifndef MPCQP_POLY_LOOP_REBUILD
#define MPCQP_POLY_LOOP_REBUILD 64
#endif

namespace mpcqp {

constexpr int kPolyLoopRebuild = MPCQP_POLY_LOOP_REBUILD;

template <typename T>
struct PolyLoopArgs {
  int batch, n, m, mt, nx, nu, steps, cold;
  const T* M;                  // packed lower mt x mt
  const T* Ut;                 // mt x n
  const T* Kt;                 // nx x n
  const T* L;                  // mt x nx
  const int32_t* flag;         // set by the shared inverse when H is not PD
  const T* E;                  // m x nx or null
  const T* A; const T* B;      // plant
  const T* x0; int64_t sX0;
  const T* hl; const T* hu; int64_t sh;
  const T* lbz; const T* ubz;
  const T* w;                  // steps x batch x nx or null
  T* xs; T* us; T* zs; T* ys;
  int32_t* status;
  int max_iter;
  T tol;
};

// mpcqp_mpc_poly_loop_soft: the per-row penalties and the slack output
template <typename T>
struct PolyLoopSoftArgs : PolyLoopArgs<T> {
  const T* rho;                // m, +inf = hard row
  const T* sigma;              // m, read where rho is finite
  T* eps;                      // steps x batch x m or null
};

// mpcqp_mpc_poly_loop_affine: the products of poly_affine_prep_kernel and the
// row shift.  Row (t, b) of zg / sg is t * gB + gmul * b (shared g: gB = 1,
// gmul = 0), of e it is t * eB + emul * b.  rho is null in the hard instantiation.
template <typename T>
struct PolyLoopAffineArgs : PolyLoopSoftArgs<T> {
  const T* zg;                 // R x n: -Hinv g, or null
  const T* sg;                 // R x mt: -Ut g, or null
  const T* e;                  // steps x (batch or 1) x m, or null
  int gB, gmul, eB, emul;
};
template <typename T, bool SOFT, bool AFFINE = false>
using PolyLoopArgsOf =
    std::conditional_t<AFFINE, PolyLoopAffineArgs<T>,
                       std::conditional_t<SOFT, PolyLoopSoftArgs<T>, PolyLoopArgs<T>>>;

// LDS elements of the loop kernel: Sym2D scratch, the mat-vec partials, packed
// M, L' and E' (nx x NMAX each, transposed: lane = row reads conflict-free),
// A, B, the first nu columns of Ut (NMAX x nu) and Kt (nx x nu), x_t, u_t.
__host__ __device__ inline int poly_loop_lds(int BS, int mt, int nx, int nu) {
  const int NMAX = 8 * BS;
  return NMAX * BS + NMAX + 8 * NMAX + mt * (mt + 1) / 2 + 2 * nx * NMAX + nx * nx + nx * nu +
         NMAX * nu + nx * nu + 32;
}

// st: 0 inactive, 1 at lower, 2 at upper, 3 padding row; row-indexed vectors
// one row per lane, as in dual_range_kernel.
//
// SOFT: rows < m with a finite rho are soft (exact penalty rho eps + 1/2 sigma
// eps^2 on a slack shared by the row's two sides).  Such a row has a third
// state, "soft-active" (|y| > rho, row value = bound + sgn (|y| - rho)/sigma),
// held as the regime bit sr next to st; a soft-active row is an ordinary
// active row of the problem with M_ii + 1/sigma on its diagonal and the bound
// moved by -sgn rho/sigma, so W is SWEEP_A of that matrix and a regime switch
// of an active row is a rank-one update of W (Sym2D::update_col).
//
// AFFINE: a is a PolyLoopAffineArgs; per step the row's lane adds sg to s0,
// moves the bounds of the rows < m by -e_t, and the epilogue starts from zg.
template <typename T, int BS, bool SOFT, bool AFFINE = false>
__global__ __launch_bounds__(64) void poly_loop_kernel(PolyLoopArgsOf<T, SOFT, AFFINE> a) {
  using S2 = Sym2D<T, BS>;
  constexpr int NMAX = S2::NMAX;
  static_assert(NMAX <= kWave, "one row per lane");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int mt = a.mt, m = a.m, nz = a.n, nx = a.nx, nu = a.nu;
  const int P = mt * (mt + 1) / 2;
  T* buf = reinterpret_cast<T*>(smem_raw);
  T* part = buf + S2::BUF;
  T* Ps = part + 8 * NMAX;
  T* Lt = Ps + P;
  T* Et = Lt + nx * NMAX;
  T* As = Et + nx * NMAX;
  T* Bs = As + nx * nx;
  T* Un = Bs + nx * nu;
  T* Kn = Un + NMAX * nu;
  T* xl = Kn + nx * nu;
  T* ul = xl + 16;

  // ------------------------------------------------------------- stage in
  stage_packed<T, NMAX*(NMAX + 1) / 2>(a.M, Ps, P, lane);
  for (int e = lane; e < nx * NMAX; e += kWave) {
    const int k = e / NMAX, r = e - k * NMAX;
    Lt[e] = r < mt ? a.L[r * nx + k] : T(0);
    Et[e] = (a.E && r < m) ? a.E[r * nx + k] : T(0);
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
  if (lane < 16) {
    xl[lane] = lane < nx ? a.x0[(int64_t)b * a.sX0 + lane] : T(0);
    ul[lane] = T(0);
  }
  __syncthreads();

  // row `lane`: bounds (rows < m per instance or shared, the box rows shared), M_ii
  const bool row = lane < mt;
  T li = -Lim<T>::inf(), ui = Lim<T>::inf(), md = T(1);
  if (row) {
    if (lane < m) {
      if (a.hl) li = a.hl[(int64_t)b * a.sh + lane];
      if (a.hu) ui = a.hu[(int64_t)b * a.sh + lane];
    } else {
      if (a.lbz) li = a.lbz[lane - m];
      if (a.ubz) ui = a.ubz[lane - m];
    }
    md = Ps[lane * (lane + 1) / 2 + lane];
  }
  bool nf0 = row && (li != li || ui != ui);
  // penalties: rho (+inf on hard rows), 1/sigma (0 on hard rows), and the
  // regime of an active row: sr = soft-active
  T rho = Lim<T>::inf(), isg = T(0);
  bool sr = false;
  if constexpr (SOFT) {
    if (lane < m) {
      rho = a.rho[lane];
      nf0 |= !(rho >= T(0));
      if (rho < Lim<T>::inf()) {
        const T sg = a.sigma[lane];
        nf0 |= !(sg > T(0) && sg < Lim<T>::inf());
        isg = T(1) / sg;
      }
    }
  }
  for (int e = lane; e < P; e += kWave) nf0 |= !finite(Ps[e]);
  const bool badbox =
      row && (!(li <= ui) || li == Lim<T>::inf() || ui == -Lim<T>::inf());
  // NONFINITE, then INFEASIBLE, then NOT_CONVEX
  const int code0 = __any(nf0) ? MPCQP_STATUS_NONFINITE
                    : __any(badbox) ? MPCQP_STATUS_INFEASIBLE
                    : *a.flag ? MPCQP_STATUS_NOT_CONVEX
                              : MPCQP_STATUS_OPTIMAL;

  S2 W;
  W.init(lane);
  int st = row ? 0 : 3;
  T yi = T(0), si = T(0);
  const T tol = a.tol;
  constexpr T dep_tol = kDualDepTol<T>;
  const int max_iter = a.max_iter;
  int failed = MPCQP_STATUS_OPTIMAL;  // code of the instance's first failed step
  bool reload = true;                 // W <- M at the top of the step ...
  uint64_t rmask = 0;                 // ... then these rows swept back in
  bool fresh = false;                 // W is exactly M
  int since = 0;                      // steps since W was last loaded from M

  for (int t = 0; t < a.steps; ++t) {
    const int64_t tb = (int64_t)t * a.batch + b;
    // record x_t; the step's disturbance; s0 = L x_t, the rows' shift E x_t
    T wv = T(0);
    bool nf = false;
    int64_t rg = 0;  // AFFINE: the step's row of zg / sg
    if constexpr (AFFINE) rg = (int64_t)t * a.gB + (int64_t)a.gmul * b;
    if (lane < nx) {
      const T xv = xl[lane];
      a.xs[tb * nx + lane] = xv;
      if (a.w) wv = a.w[tb * nx + lane];
      nf = !finite(xv) || !finite(wv);
    }
    T s0 = T(0), ex = T(0);
    if (row) {
      for (int k = 0; k < nx; ++k) {
        const T xk = xl[k];
        s0 = fma(Lt[k * NMAX + lane], xk, s0);
        ex = fma(Et[k * NMAX + lane], xk, ex);
      }
      nf |= !finite(s0) || !finite(ex);
    }
    T lt = li - ex, ut = ui - ex;
    if constexpr (AFFINE) {
      // loaded here, not ahead of the L x_t products: two values less in flight
      // keep the BS = 2 hard instantiation at 4 waves per SIMD (126 VGPRs, not 130)
      T sgv = T(0), ev = T(0);
      if (a.sg && row) sgv = a.sg[rg * mt + lane];
      if (a.e && lane < m) ev = a.e[((int64_t)t * a.eB + (int64_t)a.emul * b) * m + lane];
      nf |= !finite(sgv) || !finite(ev);
      s0 += sgv;
      lt -= ev;
      ut -= ev;
    }
    // relative-violation scales 1/(1+|bound|), NaN for an infinite bound (a NaN
    // violation never wins the arg-max)
    const T sl = finite(lt) ? T(1) / (T(1) + fabs(lt)) : T(__builtin_nan(""));
    const T su = finite(ut) ? T(1) / (T(1) + fabs(ut)) : T(__builtin_nan(""));

    int code = __any(nf) ? MPCQP_STATUS_NONFINITE : code0;
    if (failed != MPCQP_STATUS_OPTIMAL) code = failed;
    int iters = 0;
    yi = T(0);

    if (code == MPCQP_STATUS_OPTIMAL) {
      if (reload) {
        bool unused = false;
        W.load_packed(Ps, mt, unused);
        fresh = rmask == 0;
        since = 0;
      }
      // w = (s0 - b on active rows, 0 elsewhere);  v = W w;
      // active: y = -v, s = bound;  inactive: s = s0 - v
      auto refresh = [&]() {
        const bool act = st == 1 || st == 2;
        T bnd = (st == 1) ? lt : ut;
        if constexpr (SOFT) {
          if (sr) bnd -= ((st == 1) ? -rho : rho) * isg;
        }
        const T v = matvec_lane_lds<T, BS>(W, act ? s0 - bnd : T(0), buf, part);
        yi = act ? -v : T(0);
        si = act ? bnd : s0 - v;
      };
      // phase 0: sweep the rows of rmask back into the reloaded W;
      // phase 1: drop the active rows whose multiplier has the wrong sign;
      // phase 2: the dual range active set of dual_range_kernel
      int phase = rmask ? 0 : 1;
      if (phase == 1) refresh();
      bool havep = false;
      int p = 0, side = 0;
      T sp = T(0), tgt = T(0), ysgn = T(0), mpp = T(1);
      // SOFT, for the entering row p: its penalties, |y_p| so far, and whether
      // it has passed rho (then sp is its row value less the slack)
      T rhop = Lim<T>::inf(), isgp = T(0), yp = T(0);
      bool psoft = false;
      code = MPCQP_STATUS_MAXITER;
      while (true) {
        int idx = 0;
        T sig = T(1), d = T(1), dd = T(0);
        bool r1 = false;
        T c[BS], cc[BS];
        bool add = false, op = false, stop = false;
        // choose the next sweep; W is only read in here, so that the loop
        // that rewrites it has the sweep as its one definition of W
        while (!op && !stop) {
          if (phase == 0) {
            if (!rmask) {
              phase = 1;
              refresh();
            } else {
              idx = uniform(__builtin_ctzll(rmask));
              rmask &= rmask - 1;
              ++iters;
              d = W.column(idx, buf, c, cc);
              if constexpr (SOFT) d += readlane(sr ? isg : T(0), idx);
              if (d > T(0)) {
                op = true;
              } else if (lane == idx) {  // cannot happen for a set that was swept in before
                st = 0;
                sr = false;
              }
            }
          } else if (phase == 1) {
            T wrong = (st == 2) ? -yi : ((st == 1) ? yi : -Lim<T>::inf());
            if constexpr (SOFT) {
              // ... or whose |y| is on the wrong side of rho for its regime
              if (st == 1 || st == 2) wrong = sr ? rho + wrong : fmax(wrong, -wrong - rho);
            }
            const T wmax = wave_max(wrong);
            if (!(readlane(wmax, 0) > T(0))) {
              phase = 2;
            } else if (++iters > max_iter) {
              stop = true;
            } else {
              const uint64_t kb = __builtin_amdgcn_ballot_w64(wrong == wmax);
              idx = kb ? uniform(__builtin_ctzll(kb)) : 0;
              if constexpr (SOFT) dd = readlane(sr ? -isg : T(0), idx);
              if (lane == idx) {
                st = row ? 0 : 3;
                yi = T(0);
                sr = false;
              }
              sig = T(-1);
              d = W.column(idx, buf, c, cc);
              op = true;
            }
          } else {
            if (!havep) {
              const T vl = (lt - si) * sl;
              const T vu = (si - ut) * su;
              const T viol = (st == 0) ? fmax(vl, vu) : -Lim<T>::inf();
              const T vmax = wave_max(viol);
              if (!(readlane(vmax, 0) > tol)) {
                code = MPCQP_STATUS_OPTIMAL;
                stop = true;
              } else {
                const uint64_t pb = __builtin_amdgcn_ballot_w64(viol == vmax);
                p = pb ? uniform(__builtin_ctzll(pb)) : 0;
                sp = readlane(si, p);
                const T lp = readlane(lt, p), up = readlane(ut, p);
                mpp = readlane(md, p);
                side = (sp < lp) ? 1 : 2;
                tgt = (side == 1) ? lp : up;
                ysgn = (side == 1) ? T(-1) : T(1);
                havep = true;
                if constexpr (SOFT) {
                  rhop = readlane(rho, p);
                  isgp = readlane(isg, p);
                  yp = T(0);
                  psoft = !(rhop > T(0));
                }
              }
            }
            if (!stop && ++iters > max_iter) stop = true;
            if (!stop) {
              if constexpr (SOFT) {
                T cl;
                const T wpp0 = W.template column<true>(p, buf, c, cc, cl);  // cl = W_lane,p
                // past rho the row's pivot carries its 1/sigma
                const T wpp = psoft ? wpp0 + isgp : wpp0;
                const T mref = psoft ? mpp + isgp : mpp;
                const bool dep = !(wpp > dep_tol * fmax(mref, T(1e-300)));
                // an active row's multiplier moves toward 0: t = -y / dy (>= 0)
                const T dy = -cl * ysgn;
                // Along the ray of a dependent row p only the rows that p depends on
                // move: cl = 0 elsewhere, exactly so while W is M swept, but left as
                // rounding noise by the 1/sigma updates, and no bound on the step
                // hides an event at -y / noise.  With a soft-active row in the set,
                // a row moves if its share |cl| sqrt(M_ii) of row p's norm passes
                // dep_tol.
                const bool ray = dep && __any(sr);
                const bool moves =
                    !ray || cl * cl * md > dep_tol * dep_tol * fmax(mref, T(1e-300));
                const bool cand = moves && ((st == 2 && dy < T(0)) || (st == 1 && dy > T(0)));
                T tl = cand ? -yi * fast_rcp(dy) : Lim<T>::inf();
                int kind = 0;  // of this lane's event: 0 drop, 1 to soft-active, 2 back to hard-active
                const T ady = fabs(dy);
                if (cand && sr) {  // |y| shrinks to rho first
                  tl = fmax(fabs(yi) - rho, T(0)) * fast_rcp(ady);
                  kind = 2;
                } else if (!cand && moves && (st == 1 || st == 2) && !sr && rho < Lim<T>::inf() &&
                           ady > T(0)) {  // |y| grows to rho
                  tl = fmax(rho - fabs(yi), T(0)) * fast_rcp(ady);
                  kind = 1;
                }
                const T ti = readlane(wave_min(tl), 0);
                const uint64_t kb = __builtin_amdgcn_ballot_w64(tl == ti);
                const int k = kb ? uniform(__builtin_ctzll(kb)) : 0;
                const T t2 = dep ? Lim<T>::inf() : fabs(sp - tgt) / wpp;
                // |y_p| reaches rho_p before the row reaches its bound
                const T t3 = !psoft ? rhop - yp : Lim<T>::inf();
                if (!(ti < Lim<T>::inf()) && !(t2 < Lim<T>::inf()) && !(t3 < Lim<T>::inf())) {
                  code = MPCQP_STATUS_INFEASIBLE;
                  stop = true;
                } else if (ti < t2 && ti < t3) {  // wave-uniform: a partial step to row k's event
                  if (st == 1 || st == 2) yi = fma(ti, dy, yi);
                  if (!dep) sp = sp - wpp * ysgn * ti;
                  const int kk = uniform(readlane(kind, k));
                  idx = k;
                  d = W.column(k, buf, c, cc);
                  if (kk == 0) {
                    if (lane == k) {
                      yi = T(0);
                      st = row ? 0 : 3;
                    }
                    sig = T(-1);
                  } else {  // regime switch of row k at |y_k| = rho_k: M_kk -+ 1/sigma_k
                    const T dl = readlane(kk == 1 ? isg : -isg, k);
                    const T den = T(1) - dl * d;  // >= 1 towards soft, in [0, 1] back to hard
                    if (den > dep_tol) {
                      if (lane == k) {
                        yi = (st == 1) ? -rho : rho;
                        sr = kk == 1;
                      }
                      d = dl / den;
                      r1 = true;
                    } else {
                      // as a hard row k depends on the rest of the set (a velocity row
                      // next to the input bound that fixes it): it cannot stay.  It
                      // leaves, and the step starts over from the repair with the set
                      // that is left.
                      if (lane == k) {
                        yi = T(0);
                        st = row ? 0 : 3;
                        sr = false;
                      }
                      dd = dl;
                      sig = T(-1);
                      phase = 1;
                      havep = false;
                    }
                  }
                  yp += ti;
                  op = true;
                } else if (t3 < t2) {  // row p goes on as a soft row; W is not touched
                  if (st == 1 || st == 2) yi = fma(t3, dy, yi);
                  if (!dep) sp = sp - wpp * ysgn * t3;
                  yp = rhop;
                  psoft = true;
                } else if (!(wpp > T(0))) {
                  code = MPCQP_STATUS_NOT_CONVEX;
                  stop = true;
                } else {
                  idx = p;
                  sig = T(1);
                  d = wpp;
                  add = op = true;
                }
              } else {
                T cl;
                const T wpp = W.template column<true>(p, buf, c, cc, cl);  // cl = W_lane,p
                const bool dep = !(wpp > dep_tol * fmax(mpp, T(1e-300)));
                // an active row's multiplier moves toward 0: t = -y / dy (>= 0)
                const T dy = -cl * ysgn;
                const bool cand = (st == 2 && dy < T(0)) || (st == 1 && dy > T(0));
                const T tl = cand ? -yi * fast_rcp(dy) : Lim<T>::inf();
                const T ti = readlane(wave_min(tl), 0);
                const uint64_t kb = __builtin_amdgcn_ballot_w64(tl == ti);
                const int k = kb ? uniform(__builtin_ctzll(kb)) : 0;
                const T t2 = dep ? Lim<T>::inf() : fabs(sp - tgt) / wpp;
                if (!(ti < Lim<T>::inf()) && !(t2 < Lim<T>::inf())) {
                  code = MPCQP_STATUS_INFEASIBLE;
                  stop = true;
                } else if (ti < t2) {  // wave-uniform: a partial step that drops row k
                  if (st == 1 || st == 2) yi = fma(ti, dy, yi);
                  if (lane == k) {
                    yi = T(0);
                    st = row ? 0 : 3;
                  }
                  if (!dep) sp = sp - wpp * ysgn * ti;
                  idx = k;
                  sig = T(-1);
                  d = W.column(k, buf, c, cc);
                  op = true;
                } else if (!(wpp > T(0))) {
                  code = MPCQP_STATUS_NOT_CONVEX;
                  stop = true;
                } else {
                  idx = p;
                  sig = T(1);
                  d = wpp;
                  add = op = true;
                }
              }
            }
          }
        }
        if (stop) break;
        if constexpr (SOFT) {
          W.update_col(idx, sig, d, r1, dd, c, cc);
        } else {
          W.sweep_col(idx, sig, d, c, cc);
        }
        fresh = false;
        if (phase == 1) refresh();
        if (add) {
          if (lane == p) {
            st = side;
            sr = psoft;
          }
          refresh();
          havep = false;
        }
      }
    }

    const bool okc = code == MPCQP_STATUS_OPTIMAL || code == MPCQP_STATUS_MAXITER;
    if (!okc) {
      failed = code;
      yi = T(__builtin_nan(""));
    }
    if (a.ys && row) a.ys[tb * mt + lane] = yi;
    const uint64_t yact = __builtin_amdgcn_ballot_w64(row && yi != T(0));
    // the applied input from the LDS columns; the plan from the global factors
    {
      const int j = lane < nu ? lane : 0;
      T z0 = T(0);
      if constexpr (AFFINE) {
        if (a.zg) z0 = a.zg[rg * nz + j];
      }
      const T uv = poly_epilogue<T>(Kn, Un, nu, j, nx, xl, yi, yact, z0);
      if (lane < nu) {
        const T uo = okc ? uv : T(__builtin_nan(""));
        ul[lane] = uo;
        a.us[tb * nu + lane] = uo;
      }
    }
    if (a.zs) {
      for (int j0 = 0; j0 < nz; j0 += kWave) {
        const int j = j0 + lane;
        T z0 = T(0);
        if constexpr (AFFINE) {
          if (a.zg) z0 = a.zg[rg * nz + (j < nz ? j : 0)];
        }
        const T zv = poly_epilogue<T>(a.Kt, a.Ut, nz, j < nz ? j : 0, nx, xl, yi, yact, z0);
        if (j < nz) a.zs[tb * nz + j] = okc ? zv : T(__builtin_nan(""));
      }
    }
    int word = (code & 0xff) | ((iters & 0xffff) << 8);
    if constexpr (SOFT) {
      // the slack of a soft-active row; bit 26 when the step ends with one
      T ev = (sr && (st == 1 || st == 2)) ? fmax((fabs(yi) - rho) * isg, T(0)) : T(0);
      if (!okc) ev = T(__builtin_nan(""));
      if (__any(ev > T(0))) word |= MPCQP_STATUS_SOFTENED;
      if (a.eps && lane < m) a.eps[tb * m + lane] = ev;
    }
    if (lane == 0) a.status[tb] = word;
    lds_exchange();
    // plant: x_{t+1} = A x_t + B u_t (+ w_t)
    T xn = T(0);
    if (lane < nx) {
      for (int j = 0; j < nx; ++j) xn = fma(As[lane * nx + j], xl[j], xn);
      for (int j = 0; j < nu; ++j) xn = fma(Bs[lane * nu + j], ul[j], xn);
      if (a.w) xn += wv;
    }
    lds_exchange();
    if (lane < nx) xl[lane] = xn;
    lds_exchange();

    // the next step's start: cold after a failure (or on request); W reloaded
    // when the set is empty (free, exact) and rebuilt every kPolyLoopRebuild steps
    rmask = 0;
    if (!okc || a.cold) {
      st = row ? 0 : 3;
      sr = false;
      reload = !fresh;
    } else {
      const uint64_t act = __builtin_amdgcn_ballot_w64(st == 1 || st == 2);
      ++since;
      if (!act) {
        reload = !fresh;
      } else if (since >= kPolyLoopRebuild) {
        reload = true;
        rmask = act;
      } else {
        reload = false;
      }
    }
  }
  if (lane < nx) a.xs[((int64_t)a.steps * a.batch + b) * nx + lane] = xl[lane];
}

// zg = -Hinv g (R x n) and sg = -Ut g (R x mt) for the R rows of g: the
// state-independent products of every step of mpcqp_mpc_poly_loop_affine, a
// skinny GEMM [R x n] . [n x (n + mt)].  A workgroup takes kPrepRows rows of g,
// staged kPrepK columns at a time in LDS; a thread owns one output column (a
// column of Hinv, read along its contiguous rows since Hinv is symmetric, or a
// row of Ut, staged through LDS so that the global read runs along k) and
// keeps one accumulator per tile row: an element of Hinv / Ut is loaded once
// per tile and used kPrepRows times from its register.  No atomics; every
// output element has one writer.
constexpr int kPrepRows = 16, kPrepK = 32, kPrepThreads = 256;

template <typename T>
__global__ __launch_bounds__(kPrepThreads) void poly_affine_prep_kernel(
    const T* __restrict__ g, int64_t R, int n, int mt, const T* __restrict__ Hinv,
    const T* __restrict__ Ut, T* __restrict__ zg, T* __restrict__ sg) {
  __shared__ T gs[kPrepRows][kPrepK];
  __shared__ T uts[kWave][kPrepK + 1];  // +1: lane = row reads hit distinct banks
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kPrepRows;
  for (int c0 = 0; c0 < n + mt; c0 += kPrepThreads) {
    const int c = c0 + tid;
    const bool ucols = c0 + kPrepThreads > n;  // this block of columns reaches into Ut
    T acc[kPrepRows];
#pragma unroll
    for (int i = 0; i < kPrepRows; ++i) acc[i] = T(0);
    for (int k0 = 0; k0 < n; k0 += kPrepK) {
      const int kc = min(kPrepK, n - k0);
      __syncthreads();
      for (int e = tid; e < kPrepRows * kPrepK; e += kPrepThreads) {
        const int i = e / kPrepK, kk = e - i * kPrepK;
        gs[i][kk] = (r0 + i < R && kk < kc) ? g[(r0 + i) * n + k0 + kk] : T(0);
      }
      if (ucols) {
        for (int e = tid; e < mt * kPrepK; e += kPrepThreads) {
          const int r = e / kPrepK, kk = e - r * kPrepK;
          uts[r][kk] = kk < kc ? Ut[(int64_t)r * n + k0 + kk] : T(0);
        }
      }
      __syncthreads();
      if (c < n) {
        for (int kk = 0; kk < kc; ++kk) {
          const T h = Hinv[(int64_t)(k0 + kk) * n + c];
#pragma unroll
          for (int i = 0; i < kPrepRows; ++i) acc[i] = fma(h, gs[i][kk], acc[i]);
        }
      } else if (c < n + mt) {
        for (int kk = 0; kk < kc; ++kk) {
          const T h = uts[c - n][kk];
#pragma unroll
          for (int i = 0; i < kPrepRows; ++i) acc[i] = fma(h, gs[i][kk], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kPrepRows; ++i) {
      if (r0 + i < R) {
        if (c < n) zg[(r0 + i) * n + c] = -acc[i];
        else if (c < n + mt) sg[(r0 + i) * mt + (c - n)] = -acc[i];
      }
    }
  }
}

// The one launch site of poly_affine_prep_kernel (poly_prep.hpp).
int launch_poly_affine_prep(const char* who, int dtype, const void* g, int64_t R, int n, int mt,
                            const void* Hinv, const void* Ut, void* zg, void* sg,
                            hipStream_t st) {
  const int64_t blocks = (R + kPrepRows - 1) / kPrepRows;
  MPCQP_CHECK_ARG(blocks <= 0x7fffffff, "%s: %lld rows of g exceed the grid", who, (long long)R);
  auto run = [&](auto tp) {
    using T = decltype(tp);
    hipLaunchKernelGGL((poly_affine_prep_kernel<T>), dim3((unsigned)blocks), dim3(kPrepThreads),
                       0, st, (const T*)g, R, n, mt, (const T*)Hinv, (const T*)Ut, (T*)zg,
                       (T*)sg);
    MPCQP_CHECK_LAUNCH("poly_affine_prep_kernel");
    return (int)MPCQP_OK;
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}

// Scratch of mpcqp_mpc_poly_loop_affine: zg, then sg.
struct PolyAffineWs {
  int64_t R, oZg, oSg, total;
};
static inline PolyAffineWs poly_affine_ws(size_t es, int batch, int n, int mt, int steps,
                                          bool shared) {
  PolyAffineWs w;
  w.R = (int64_t)steps * (shared ? 1 : batch);
  w.oZg = 0;
  w.oSg = align256(w.R * n * (int64_t)es);
  w.total = align256(w.oSg + w.R * mt * (int64_t)es);
  return w;
}

template <typename T, int BS, bool SOFT, bool AFFINE>
static int launch_poly_loop(const PolyLoopArgsOf<T, SOFT, AFFINE>& a, hipStream_t st) {
  const size_t bytes = (size_t)poly_loop_lds(BS, a.mt, a.nx, a.nu) * sizeof(T);
  if (bytes > 64 * 1024) {
    set_error("mpcqp_mpc_poly_loop: %zu B of LDS needed, 65536 available", bytes);
    return MPCQP_ENOTSUP;
  }
  hipLaunchKernelGGL((poly_loop_kernel<T, BS, SOFT, AFFINE>), dim3((unsigned)a.batch),
                     dim3(kWave), bytes, st, a);
  MPCQP_CHECK_LAUNCH("poly_loop_kernel");
  return MPCQP_OK;
}

template <typename T, bool SOFT, bool AFFINE = false>
static int poly_loop_t(const PolyLoopArgsOf<T, SOFT, AFFINE>& a, hipStream_t st) {
  return dispatch_bs<8>(a.mt, [&](auto bs) {
    return launch_poly_loop<T, decltype(bs)::value, SOFT, AFFINE>(a, st);
  });
}

// All three entry points: rho == nullptr is the hard loop; g == e == nullptr
// launches the kernels of the first two.
static int poly_loop_entry(const char* who, int dtype, int batch, int n, int m, int nbox, int nx,
                           int nu, int steps, int flags, const void* workspace, const void* E,
                           const void* A, const void* Bm, const void* x0, int64_t strideX0,
                           const void* hl, const void* hu, int64_t strideh, const void* lbz,
                           const void* ubz, const void* w, const void* rho, const void* sigma,
                           void* xs, void* us, void* zs, void* ys, void* eps, int32_t* status,
                           int max_iter, double tol, void* stream, const void* g = nullptr,
                           int64_t strideG = 0, const void* e = nullptr, int64_t strideE = 0,
                           void* scratch = nullptr, size_t scratch_bytes = 0) {
  MPCQP_CHECK_ARG(dtype == MPCQP_F64 || dtype == MPCQP_F32, "%s: bad dtype %d", who, dtype);
  MPCQP_CHECK_ARG(batch >= 0 && n >= 1 && m >= 0 && steps >= 0,
                  "%s: bad sizes batch=%d n=%d m=%d steps=%d", who, batch, n, m, steps);
  MPCQP_CHECK_ARG(m + (nbox ? n : 0) >= 1 && m + (nbox ? n : 0) <= 64,
                  "%s: rows m_total=%d outside [1,64]", who, m + (nbox ? n : 0));
  MPCQP_CHECK_ARG(nx >= 1 && nx <= 16 && nu >= 1 && nu <= 16 && nu <= n,
                  "%s: nx=%d nu=%d outside 1 <= nx <= 16, 1 <= nu <= min(16, n)", who, nx, nu);
  MPCQP_CHECK_ARG(workspace && A && Bm && x0 && xs && (steps == 0 || (us && status)),
                  "%s: workspace, A, B, x0, xs (and us, status for steps > 0) are required", who);
  MPCQP_CHECK_ARG(strideX0 >= 0 && strideh >= 0, "%s: negative stride", who);
  MPCQP_CHECK_ARG(!nbox || lbz || ubz, "%s: nbox set without lbz/ubz", who);
  MPCQP_CHECK_ARG(!rho || sigma, "%s: rho given without sigma", who);
  MPCQP_CHECK_ARG(strideG >= 0 && strideE >= 0, "%s: negative stride", who);
  MPCQP_CHECK_ARG(!g || strideG == 0 || strideG == n, "%s: strideG=%lld is neither 0 nor n=%d",
                  who, (long long)strideG, n);
  MPCQP_CHECK_ARG(!e || strideE == 0 || strideE == m, "%s: strideE=%lld is neither 0 nor m=%d",
                  who, (long long)strideE, m);
  const int mt = m + (nbox ? n : 0);
  const PolyAffineWs S = poly_affine_ws(dtype_size(dtype), batch, n, mt, steps, strideG == 0);
  MPCQP_CHECK_ARG(!g || S.total == 0 || (scratch && scratch_bytes >= (size_t)S.total),
                  "%s: g needs %lld B of scratch, %zu given", who, (long long)S.total,
                  scratch ? scratch_bytes : (size_t)0);
  if (batch == 0) return MPCQP_OK;
  const PolyWs L = poly_ws(dtype_size(dtype), n, mt, nx);
  const char* base = (const char*)workspace;
  auto fill = [&](auto& a, auto tp) {
    using T = decltype(tp);
    a.batch = batch; a.n = n; a.m = m; a.mt = mt; a.nx = nx; a.nu = nu; a.steps = steps;
    a.cold = (flags & MPCQP_LOOP_COLD) ? 1 : 0;
    a.M = (const T*)(base + L.oM); a.Ut = (const T*)(base + L.oUt);
    a.Kt = (const T*)(base + L.oKt); a.L = (const T*)(base + L.oL);
    a.flag = (const int32_t*)(base + L.oFlag);
    a.E = (const T*)E; a.A = (const T*)A; a.B = (const T*)Bm;
    a.x0 = (const T*)x0; a.sX0 = strideX0;
    a.hl = (const T*)hl; a.hu = (const T*)hu; a.sh = strideh;
    a.lbz = nbox ? (const T*)lbz : nullptr; a.ubz = nbox ? (const T*)ubz : nullptr;
    a.w = (const T*)w;
    a.xs = (T*)xs; a.us = (T*)us; a.zs = (T*)zs; a.ys = (T*)ys; a.status = status;
    a.max_iter = dual_max_iter(max_iter, mt);
    a.tol = dual_tol<T>(tol);
  };
  auto run = [&](auto tp) {
    using T = decltype(tp);
    hipStream_t st = (hipStream_t)stream;
    if ((g || (e && m > 0)) && steps > 0) {
      PolyLoopAffineArgs<T> a;
      fill(a, tp);
      a.rho = (const T*)rho; a.sigma = (const T*)sigma; a.eps = rho ? (T*)eps : nullptr;
      a.zg = a.sg = nullptr;
      a.gB = strideG == 0 ? 1 : batch; a.gmul = strideG == 0 ? 0 : 1;
      a.e = m > 0 ? (const T*)e : nullptr;
      a.eB = strideE == 0 ? 1 : batch; a.emul = strideE == 0 ? 0 : 1;
      if (g) {
        T* zg = (T*)((char*)scratch + S.oZg);
        T* sg = (T*)((char*)scratch + S.oSg);
        const int rc = launch_poly_affine_prep(who, dtype, g, S.R, n, mt, base + L.oHinv,
                                               base + L.oUt, zg, sg, st);
        if (rc != MPCQP_OK) return rc;
        a.zg = zg; a.sg = sg;
      }
      return rho ? poly_loop_t<T, true, true>(a, st) : poly_loop_t<T, false, true>(a, st);
    }
    if (rho) {
      PolyLoopSoftArgs<T> a;
      fill(a, tp);
      a.rho = (const T*)rho; a.sigma = (const T*)sigma; a.eps = (T*)eps;
      return poly_loop_t<T, true>(a, st);
    }
    PolyLoopArgs<T> a;
    fill(a, tp);
    return poly_loop_t<T, false>(a, st);
  };
  return dtype == MPCQP_F64 ? run(0.0) : run(0.0f);
}

}  // namespace mpcqp

extern "C" int mpcqp_mpc_poly_loop(int dtype, int batch, int n, int m, int nbox, int nx, int nu,
                                   int steps, int flags, const void* workspace, const void* E,
                                   const void* A, const void* Bm, const void* x0,
                                   int64_t strideX0, const void* hl, const void* hu,
                                   int64_t strideh, const void* lbz, const void* ubz,
                                   const void* w, void* xs, void* us, void* zs, void* ys,
                                   int32_t* status, int max_iter, double tol, void* stream) {
  return mpcqp::poly_loop_entry("mpcqp_mpc_poly_loop", dtype, batch, n, m, nbox, nx, nu, steps,
                                flags, workspace, E, A, Bm, x0, strideX0, hl, hu, strideh, lbz, ubz,
                                w, nullptr, nullptr, xs, us, zs, ys, nullptr, status, max_iter, tol,
                                stream);
}

extern "C" int mpcqp_mpc_poly_loop_soft(int dtype, int batch, int n, int m, int nbox, int nx,
                                        int nu, int steps, int flags, const void* workspace,
                                        const void* E, const void* A, const void* Bm,
                                        const void* x0, int64_t strideX0, const void* hl,
                                        const void* hu, int64_t strideh, const void* lbz,
                                        const void* ubz, const void* w, const void* rho,
                                        const void* sigma, void* xs, void* us, void* zs, void* ys,
                                        void* eps, int32_t* status, int max_iter, double tol,
                                        void* stream) {
  return mpcqp::poly_loop_entry("mpcqp_mpc_poly_loop_soft", dtype, batch, n, m, nbox, nx, nu,
                                steps, flags, workspace, E, A, Bm, x0, strideX0, hl, hu, strideh,
                                lbz, ubz, w, rho, sigma, xs, us, zs, ys, eps, status, max_iter, tol,
                                stream);
}

extern "C" size_t mpcqp_mpc_poly_loop_affine_workspace(int dtype, int batch, int n, int m, int nbox,
                                                       int steps, int g_shared) {
  if ((dtype != MPCQP_F64 && dtype != MPCQP_F32) || batch < 0 || n < 1 || m < 0 || steps < 0)
    return 0;
  return (size_t)mpcqp::poly_affine_ws(mpcqp::dtype_size(dtype), batch, n, m + (nbox ? n : 0),
                                       steps, g_shared != 0)
      .total;
}

extern "C" int mpcqp_mpc_poly_loop_affine(
    int dtype, int batch, int n, int m, int nbox, int nx, int nu, int steps, int flags,
    const void* workspace, const void* E, const void* A, const void* Bm, const void* x0,
    int64_t strideX0, const void* hl, const void* hu, int64_t strideh, const void* lbz,
    const void* ubz, const void* w, const void* rho, const void* sigma, const void* g,
    int64_t strideG, const void* e, int64_t strideE, void* scratch, size_t scratch_bytes, void* xs,
    void* us, void* zs, void* ys, void* eps, int32_t* status, int max_iter, double tol,
    void* stream) {
  return mpcqp::poly_loop_entry("mpcqp_mpc_poly_loop_affine", dtype, batch, n, m, nbox, nx, nu,
                                steps, flags, workspace, E, A, Bm, x0, strideX0, hl, hu, strideh,
                                lbz, ubz, w, rho, sigma, xs, us, zs, ys, eps, status, max_iter, tol,
                                stream, g, strideG, e, strideE, scratch, scratch_bytes);
}
