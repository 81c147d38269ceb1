// gi_box_core.hpp -- the Goldfarb-Idnani dual active set for
//     min 1/2 z'Hz + f'z   s.t.  lb <= z <= ub
// on a symmetric matrix held in registers: one QP per wavefront (Sym2D,
// sym2d.hpp: solve_box.hip, mpc_box.hip) or four (QSym, quad.hpp: quad_box.hip,
// loop_box.hip).  The layouts provide column / sweep_col / matvec and their
// reductions; everything else of the method is here.
//
// Entry state: M holds SWEEP_all(H) = -H^{-1} (all variables free), the LDS
// vectors fs/lbs/ubs hold f, lb, ub by row index (padding rows: f = 0,
// bounds = -/+inf).  On exit zr holds the solution in the row-block layout
// and the status code is returned.
//
// One iteration of the method (bound p, the most violated free variable):
//   direction  dz_F = M_{F,p} / M_pp  per unit move of z_p          (column p)
//   multiplier rates of active bounds  dmu_A = -/+ M_{A,p} / M_pp
//   partial step (a multiplier hits 0): drop that bound  -> sweep(k, +1)
//   full step (z_p reaches its bound):  add bound p       -> sweep(p, -1)
// with the primal/dual state tracked along the steps and one exact mat-vec
// refresh + re-check at the end (gi_box_st below).
//
// In order: the LDS block and the bounds, the fp64 key, row ownership
// (RowOwn), the two selection strategies (SelCmp, SelKey), gi_box_st.
#pragma once
#include <type_traits>

#include "quad.hpp"

namespace mpcqp {

// Occupancy target: 4 waves/SIMD (16 per CU) up to BS = 3 (n <= 24), which
// keeps a 4096-instance batch resident in one pass over the 256 CUs.
template <int BS>
struct BoxOcc {
  static constexpr int w = BS <= 3 ? 4 : (BS <= 5 ? 2 : 1);
};

// Keyed reductions (Key below): which layouts reduce the scan, the ratio test
// and the warm-start release scan on one fp64 key instead of a (value, index,
// payload) triple.  fp64 only: in fp32 the index bits would make values within
// 2^-18 relative compare equal.
// MPCQP_KEYED_REDUCE=0 builds the compare-and-select reductions everywhere (A/B).
#ifndef MPCQP_KEYED_REDUCE
#define MPCQP_KEYED_REDUCE 1
#endif
template <class Mat>
struct QKeyed {
  static constexpr bool v = false;
};
template <int BS>
struct QKeyed<QSym<double, BS>> {
  static constexpr bool v = MPCQP_KEYED_REDUCE != 0;
};

// LDS block of one QP (per group / per wave, T elements): [Mat::BUF | f | lb |
// ub | z], the vectors indexed by (padded) row; oBuf = 0, so the tile pointer
// gb is the block's base.  z (keyed layouts only, otherwise empty) is the
// owners' copy of the primal iterate, from which a new pivot reads z_p.
// Kernels append their own staging at oEnd.
template <class Mat>
struct BoxLds {
  static constexpr int NMAX = Mat::NMAX;
  static constexpr int NV = Mat::NV;
  static constexpr int oBuf = 0;
  static constexpr int oF = Mat::BUF;
  static constexpr int oLb = oF + NV;
  static constexpr int oUb = oLb + NV;
  static constexpr int oZ = oUb + NV;
  static constexpr int oEnd = oZ + (QKeyed<Mat>::v ? NV : 0);
};

// Relative-violation scale of a bound: 1/(1+|b|) for a finite bound, NaN for
// an infinite one (a NaN violation never wins the arg-max and fmax skips it),
// so the per-iteration scan multiplies instead of dividing.
template <typename T>
__device__ __forceinline__ T bound_scale(T bnd) {
  return finite(bnd) ? T(1) / (T(1) + fabs(bnd)) : __builtin_nan("");
}

// Bounds of this lane's rows and their violation scales, held in registers
// for the whole solve (loop-invariant; the scan runs every iteration).
template <typename T, int RO>
struct QBounds {
  T lo[RO], hi[RO], sl[RO], su[RO];
  // mi: the rows of this lane's slots (RowOwn::mrow)
  __device__ __forceinline__ void load(const int (&mi)[RO], const T* lbs, const T* ubs) {
#pragma unroll
    for (int s = 0; s < RO; ++s) {
      lo[s] = lbs[mi[s]];
      hi[s] = ubs[mi[s]];
      sl[s] = bound_scale(lo[s]);
      su[s] = bound_scale(hi[s]);
    }
  }
};

// ------------------------------------------------------------ the fp64 key
// The order of the arg-reductions (arg_step: value, then the smaller index)
// fits in one fp64 key: the low KB = ceil(log2 NMAX) mantissa bits of the
// value are replaced by a code of the row index, and a reduction step is two
// DPP moves and one v_max_f64 / v_min_f64 instead of the moves, compares and
// selects of a (value, index, payload) triple.
//   arg-max of positive values   code = 2^KB-1-idx  (larger key = smaller index)
//   arg-min of non-negative ones code = idx
//   arg-min of negative ones     code = 2^KB-1-idx  (the magnitude grows with the code)
// Values that are exactly equal resolve to the smaller index, as before;
// values that differ only in the low KB bits (2^-47 relative at KB = 5) now
// compare equal and resolve to the smaller index too.  A key must be finite
// (index bits in an infinity make a NaN): non-candidates and infinite or NaN
// values map to -/+ big(), the largest finite value with its low bits clear,
// before packing; with any code a sentinel still orders below (above) every
// candidate.  The value that comes out of a reduction has its low bits clear.
constexpr int key_bits(int nmax) {
  int b = 0;
  while ((1 << b) < nmax) ++b;
  return b;
}
template <int KB>
struct Key {
  static constexpr long long MASK = (1ll << KB) - 1;
  static __device__ __forceinline__ double clear(double v) {
    return __longlong_as_double(__double_as_longlong(v) & ~MASK);
  }
  static __device__ __forceinline__ double pack(double v, int code) {
    return __longlong_as_double((__double_as_longlong(v) & ~MASK) | (long long)(unsigned)code);
  }
  static __device__ __forceinline__ int code(double key) {
    return (int)(__double_as_longlong(key) & MASK);
  }
  static __device__ __forceinline__ double big() {
    return __longlong_as_double(0x7fefffffffffffffll & ~MASK);
  }
};
// Max / min of two keys.  A key comes out of integer operations and DPP moves,
// so the compiler cannot know that it is no signalling NaN and puts a
// canonicalising v_max_f64 x, x in front of every fmax / fmin of one: one more
// dependent fp64 instruction per reduction step.  Keys are finite by
// construction, so the bare instruction is the same function of them.
// MPCQP_KEY_BARE=0 builds fmax / fmin (A/B: config 2, 0.04487 -> 0.04425 ms per
// step, ranges 0.04480-0.04496 and 0.04417-0.04427, results bit-identical).
#ifndef MPCQP_KEY_BARE
#define MPCQP_KEY_BARE 1
#endif
__device__ __forceinline__ double key_max(double a, double b) {
#if MPCQP_KEY_BARE
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return fmax(a, b);
#endif
}
__device__ __forceinline__ double key_min(double a, double b) {
#if MPCQP_KEY_BARE
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return fmin(a, b);
#endif
}
// one reduction step on a key over DPP pattern CTRL
template <bool MAX, int CTRL>
__device__ __forceinline__ void key_step(double& key) {
  const double o = dpp<CTRL>(key);
  key = MAX ? key_max(key, o) : key_min(key, o);
}

// ----------------------------------------------------------- row ownership
// Which lanes hold the row-indexed vectors of the box active set (z, the
// multipliers, the states, the bounds and their scales).
//   replicated  every lane of a row block holds all BS rows of the block and
//               runs the scan, the ratio test and the updates over all of them
//               (one QP per wave, Sym2D: 8 lanes per row block);
//   owned       row r of a row block belongs to one lane (QSym: bj = r mod 4),
//               RO = ceil(BS / 4) slots per lane; a slot without a row is
//               padding (state 3, never a candidate, row() = -1).  Each row
//               takes the arithmetic it takes replicated, on one lane instead
//               of four, and the reductions run over all 16 lanes of the group
//               with the same order (value, then the smaller index), so the
//               results are the same bits.
// Callers keep the replicated z / states at entry and exit: the owned policy
// converts once per solve (deal() / gather()), the replicated one works on the
// caller's arrays.
// MPCQP_ROW_OWNER=0 builds the replicated layout everywhere (A/B).
#ifndef MPCQP_ROW_OWNER
#define MPCQP_ROW_OWNER 1
#endif
template <class Mat>
struct QRowOwned {
  static constexpr bool v = false;
};
// Owned at every BS.  At fp32 BS = 6 the compiler then spends more of the 256
// registers of the kernels' two-wave launch bound (box_quad_kernel 167 -> 196
// VGPRs, mpc_group_kernel 166..167 -> 191..192; the registers alone would have
// allowed 3 waves) and is faster all the same: B = 4096, n = 22, us per launch,
// replicated -> owned: nx = 2 nu = 1 68.1 -> 64.2, nx = 2 nu = 2 time-varying
// 57.2 -> 54.0, nx = 4 nu = 1 84.0 -> 82.3, nx = 4 nu = 2 time-varying 73.6 ->
// 70.0, mpcqp_solve_box 62.3 -> 57.9.
template <typename T, int BS>
struct QRowOwned<QSym<T, BS>> {
  static constexpr bool v = MPCQP_ROW_OWNER != 0;
};

// The trip of the active set on owned, keyed rows (gi_box_st): three pieces,
// each with its own switch for A/B libraries (=0 builds the tree without it).
//   MPCQP_FAST_TRIP    the ratio filter and the full-step trip
//   MPCQP_BOUND_AHEAD  the next pivot's bounds and z_p are read a trip ahead
//   MPCQP_SWEEP_RD     the sweep takes 1 / d from the trip's paths (the
//                      full-step one holds it: rm); =0 forms it behind them.
//                      Alone it does not pass the rule on the config-2 line;
//                      it stays because without it the BS = 8 shapes are
//                      slower than before the full-step trip.
#ifndef MPCQP_FAST_TRIP
#define MPCQP_FAST_TRIP 1
#endif
#ifndef MPCQP_BOUND_AHEAD
#define MPCQP_BOUND_AHEAD 1
#endif
#ifndef MPCQP_SWEEP_RD
#define MPCQP_SWEEP_RD 1
#endif
// The trip's instruction stream (layouts with QTripLean), two more pieces with
// the same kind of switch; neither changes an operand or an operation:
//   MPCQP_SWEEP_FIX  the sweep writes row k and column k as moves under lane
//                    masks instead of two select levels per entry (quad.hpp)
//   MPCQP_RATE_ONCE  the multiplier rates mu_rate(st, co * rm, sgn) are formed
//                    once per trip, in front of the filter; the filter, the
//                    ratio test and the step update read them
// Each alone gains little on the config-2 line and the two together 6 %
// (with what was measured and rejected next to them).
#ifndef MPCQP_SWEEP_FIX
#define MPCQP_SWEEP_FIX 1
#endif
#ifndef MPCQP_RATE_ONCE
#define MPCQP_RATE_ONCE 1
#endif
// Two more of the same kind, on the full-step trip's copies and waits:
//   MPCQP_FULL_SWEEP       the full-step path sweeps inside the path, on the
//                          pivot p with the column still in c / cc, 1 / d = rm
//                          and the constant sigma = -1; no copy of the column
//                          into the operands of a sweep behind the two paths,
//                          no multiply by a register that holds -1.  The
//                          sweep behind the paths serves the general one.
//   MPCQP_PUBLISH_NODRAIN  the bound read-ahead (a_lb, a_ub, a_zp) is consumed
//                          by every lane at the top of the trip, where its
//                          reads finished long ago; without that the values
//                          are pending at the pivot column's publish (their
//                          only reader is a divergent block), their registers
//                          are the column's address temporaries, and the
//                          compiler drains the publish stores before it forms
//                          the read addresses.
#ifndef MPCQP_FULL_SWEEP
#define MPCQP_FULL_SWEEP 1
#endif
#ifndef MPCQP_PUBLISH_NODRAIN
#define MPCQP_PUBLISH_NODRAIN 1
#endif
// Which layouts take them: fp64 BS = 5, the block size of the config-2 line
// they were measured on.
template <class Mat>
struct QTripLean {
  static constexpr bool v = false;
};
template <>
struct QTripLean<QSym<double, 5>> {
  static constexpr bool v = true;
};

// KEY: keyed reductions where the layout has them (QKeyed); a kernel passes
// false to keep one instantiation on the compare-and-select reductions.
// TRIP: the three pieces above where the rows are owned and keyed; a kernel
// passes false to keep one instantiation on the general trip alone.
// LEAN: the two pieces of QTripLean where the layout takes them and the
// kernel has the full-step trip; a kernel passes false to stay without them.
template <class Mat_, bool OWN_ROWS = QRowOwned<Mat_>::v, bool KEY = true, bool TRIP = true,
          bool LEAN = true>
struct RowOwn {  // replicated
  using Mat = Mat_;
  static constexpr bool OWNED = false;
  static constexpr bool KEYED = false;
  static constexpr bool FAST = false, AHEAD = false, SWEEP_RD = false;
  static constexpr bool SWEEP_FIX = false, RATE_ONCE = false;
  static constexpr bool FULL_SWEEP = false, NODRAIN = false;
  static constexpr int BS = Mat::RPL;
  static constexpr int RO = BS;
  // slot s holds a row; its matrix row, to compare with a pivot (-1: none)
  // and to address LDS
  static __device__ __forceinline__ bool has(const Mat&, int) { return true; }
  static __device__ __forceinline__ int row(const Mat& M, int s) { return M.bi * BS + s; }
  static __device__ __forceinline__ int mrow(const Mat& M, int s) { return M.bi * BS + s; }
  // arg-max / arg-min over the rows of the QP: across the row blocks
  template <bool MAX, typename T, typename... P>
  static __device__ __forceinline__ void arg(T& v, int& idx, P&... pay) {
    Mat::template rows_arg<MAX>(v, idx, pay...);
  }
  template <typename T>
  static __device__ __forceinline__ T column(Mat& M, int k, T* gb, T (&colr)[BS],
                                             T (&colc)[Mat::NC], T (&cown)[RO]) {
    const T d = M.column(k, gb, colr, colc);
#pragma unroll
    for (int r = 0; r < BS; ++r) cown[r] = colr[r];
    return d;
  }
  template <typename T>
  static __device__ __forceinline__ void matvec(Mat& M, const T (&w)[RO], T* gb, T (&out)[RO]) {
    M.matvec(w, gb, out);
  }
};

template <class Mat_, bool KEY, bool TRIP, bool LEAN>
struct RowOwn<Mat_, true, KEY, TRIP, LEAN> {  // owned (QSym)
  using Mat = Mat_;
  static constexpr bool OWNED = true;
  static constexpr int BS = Mat::RPL;
  static constexpr int RO = Mat::RO;
  static __device__ __forceinline__ bool has(const Mat& M, int s) { return M.owns(s); }
  static __device__ __forceinline__ int row(const Mat& M, int s) {
    return M.owns(s) ? M.bi * BS + M.own_row(s) : -1;
  }
  static __device__ __forceinline__ int mrow(const Mat& M, int s) {
    return M.bi * BS + M.own_mrow(s);
  }
  template <typename X>
  static __device__ __forceinline__ void deal(const Mat& M, const X (&full)[BS], X pad,
                                              X (&own)[RO]) {
#pragma unroll
    for (int s = 0; s < RO; ++s) {
      own[s] = pad;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * s + j < BS) own[s] = (M.bj == j) ? full[4 * s + j] : own[s];
    }
  }
  template <typename X>
  static __device__ __forceinline__ void gather(const Mat&, const X (&own)[RO], X (&full)[BS]) {
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      const X v = own[r / 4];
      full[r] = (r % 4 == 0)   ? quad_lane<0>(v)
                : (r % 4 == 1) ? quad_lane<1>(v)
                : (r % 4 == 2) ? quad_lane<2>(v)
                               : quad_lane<3>(v);
    }
  }
  // over the 4 owners of a row block, then over the 4 row blocks
  template <bool MAX, typename T, typename... P>
  static __device__ __forceinline__ void arg(T& v, int& idx, P&... pay) {
    Mat::template group_arg<MAX>(v, idx, pay...);
  }
  // the same reduction on one key (QKeyed)
  static constexpr bool KEYED = KEY && QKeyed<Mat>::v;
  // (=2: on the compare-and-select reductions of owned rows as well, fp32
  // included; not the default)
  static constexpr bool FAST = TRIP && (KEYED ? MPCQP_FAST_TRIP != 0 : MPCQP_FAST_TRIP == 2);
  static constexpr bool AHEAD = TRIP && (KEYED ? MPCQP_BOUND_AHEAD != 0 : MPCQP_BOUND_AHEAD == 2);
  static constexpr bool SWEEP_RD = FAST && MPCQP_SWEEP_RD != 0;
  static constexpr bool LEAN_TRIP = LEAN && FAST && KEYED && QTripLean<Mat>::v;
  static constexpr bool SWEEP_FIX = LEAN_TRIP && MPCQP_SWEEP_FIX != 0;
  static constexpr bool RATE_ONCE = LEAN_TRIP && MPCQP_RATE_ONCE != 0;
  // (the path's own sweep is the masked-move one with 1 / d handed in)
  static constexpr bool FULL_SWEEP = SWEEP_FIX && SWEEP_RD && MPCQP_FULL_SWEEP != 0;
  static constexpr bool NODRAIN = LEAN_TRIP && AHEAD && MPCQP_PUBLISH_NODRAIN != 0;
  using K = Key<key_bits(Mat::NMAX)>;
  template <bool MAX>
  static __device__ __forceinline__ void key_arg(double& key) {
    key_step<MAX, 0xB1>(key);
    key_step<MAX, 0x4E>(key);
    key_step<MAX, 0x124>(key);
    key_step<MAX, 0x128>(key);
  }
  template <typename T>
  static __device__ __forceinline__ T column(Mat& M, int k, T* gb, T (&colr)[BS],
                                             T (&colc)[Mat::NC], T (&cown)[RO]) {
    return M.column(k, gb, colr, colc, cown);
  }
  template <typename T>
  static __device__ __forceinline__ void matvec(Mat& M, const T (&w)[RO], T* gb, T (&out)[RO]) {
    M.matvec_own(w, gb, out);
  }
};

template <bool OWNED, class A, class B>
__device__ __forceinline__ auto& own_or_full(A& own, B& full) {
  if constexpr (OWNED) return own;
  else return full;
}

// ----------------------------------------------------------- the selections
// An iteration selects three times over the rows of a QP: the most violated
// free row (scan), the most negative wrong-signed multiplier of a warm start
// (release) and the first multiplier to reach zero along the step (ratio).
// Two strategies do it, chosen by Own::KEYED; both see this lane's slots:
// ri / mi = their rows (RowOwn::row / mrow), st = their states (0 free, 1 at
// lb, 2 at ub, 3 padding), zr, mu, B = their z, multipliers and bounds.

// Rate of the multiplier of a row in state st per unit step: cs = M_rp / M_pp,
// sgn = the direction z_p moves in.
template <typename T>
__device__ __forceinline__ T mu_rate(int st, T cs, T sgn) {
  return ((st == 1) ? -cs : ((st == 2) ? cs : T(0))) * sgn;
}

// The ratio filter: true when some row of this lane may block the step t2,
// decided without the reciprocal of its multiplier rate.  It must be true
// whenever ratio() below would return ti < t2; where no lane of a wave passes
// it, the trip takes the full step without running the ratio test.
//
// The ratio test finds a candidate row (active, dmu < 0) blocking when
// v(t) < t2 with t = fl(-mu * fast_rcp(dmu)) and v = Key::clear (keyed) or the
// identity.  With a = -dmu > 0:
//   fast_rcp      |r a + 1| <= 2^-51 (fp64, rcp + two Newton steps),
//                 2^-22 (fp32, rcp + one);
//   the product   one rounding, 2^-53 (2^-24);
//   Key::clear    lowers a positive t by less than 2^(KB-52) <= 2^-47 relative
//                 (KB <= 5) and never lowers a negative one;
// so v(t) < t2 implies mu < t2 a (1 + e) with e < 2^-46 (fp64) or 2^-21 (fp32).
// The filter compares mu with fl(fl(t2 (1 + DELTA)) a): two more roundings,
// 2^-52 (2^-23) together.  DELTA = 2^-40 (fp64) and 2^-16 (fp32) leave a factor
// of more than 30 over the sum.
// The bounds are relative, so they hold only away from underflow: a product
// below TINY passes the filter, and so does a step t2 outside [TINY, HUGE]
// (ratio_range; HUGE = the sentinel of the reduction, which a larger t2 or a NaN
// one would compare with).  A product that overflows is +inf and passes every
// finite mu.  A NaN multiplier fails the comparison and an infinite one is no
// smaller than any product: not blocking, as fmin(., big) / t < ti make them
// in the ratio test.
template <typename T>
struct RatioFilter;
template <>
struct RatioFilter<double> {
  static constexpr double DELTA = 0x1p-40, TINY = 0x1p-900;
};
template <>
struct RatioFilter<float> {
  static constexpr float DELTA = 0x1p-16f, TINY = 0x1p-100f;
};
// t2 (group-uniform) is in the range where the filter's bounds hold
template <typename T>
__device__ __forceinline__ bool ratio_range(T t2, T huge) {
  return t2 >= RatioFilter<T>::TINY && t2 <= huge;
}
template <typename T, int RO>
__device__ __forceinline__ bool ratio_filter(const int (&st)[RO], const T (&mu)[RO],
                                             const T (&co)[RO], T rm, T sgn, T t2) {
  const T t2d = t2 * (T(1) + RatioFilter<T>::DELTA);
  bool f = false;
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    const T dmu = mu_rate(st[r], co[r] * rm, sgn);
    const bool cand = (st[r] == 1 || st[r] == 2) && dmu < T(0);
    const T rhs = t2d * -dmu;
    f = f || (cand && (mu[r] < rhs || rhs < RatioFilter<T>::TINY));
  }
  return f;
}
// The same on rates formed once per trip (RATE_ONCE): dmu[r] is the filter's
// own mu_rate(st[r], co[r] * rm, sgn), so every word above holds unchanged.
template <typename T, int RO>
__device__ __forceinline__ bool ratio_filter(const int (&st)[RO], const T (&mu)[RO],
                                             const T (&dmu)[RO], T t2) {
  const T t2d = t2 * (T(1) + RatioFilter<T>::DELTA);
  bool f = false;
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    const bool cand = (st[r] == 1 || st[r] == 2) && dmu[r] < T(0);
    const T rhs = t2d * -dmu[r];
    f = f || (cand && (mu[r] < rhs || rhs < RatioFilter<T>::TINY));
  }
  return f;
}

// Compare-and-select on (value, index[, payload]).
template <class Own, typename T>
struct SelCmp {
  static constexpr int RO = Own::RO;
  const int (&ri)[RO];
  __device__ __forceinline__ SelCmp(const int (&ri_)[RO], const int (&)[RO], T*) : ri(ri_) {}
  // viol = the largest relative violation, pi = its row, zv = its z
  __device__ __forceinline__ void scan(const int (&st)[RO], const T (&zr)[RO],
                                       const QBounds<T, RO>& B, T& viol, int& pi, T& zv) const {
    viol = -Lim<T>::inf();
    pi = 0;
    zv = T(0);
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const T vl = (B.lo[r] - zr[r]) * B.sl[r];  // NaN for an infinite bound
      const T vu = (zr[r] - B.hi[r]) * B.su[r];
      const T v = (st[r] == 0) ? fmax(vl, vu) : -Lim<T>::inf();
      const bool take = v > viol;
      viol = take ? v : viol;
      pi = take ? ri[r] : pi;
      zv = take ? zr[r] : zv;
    }
    Own::template arg<true>(viol, pi, zv);
  }
  // k = the row to release; false: none
  __device__ __forceinline__ bool release(const int (&st)[RO], const T (&mu)[RO], T tol,
                                          int& k) const {
    T mv = Lim<T>::inf();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const bool a = (st[r] == 1 || st[r] == 2) && mu[r] < -tol;
      const bool take = a && mu[r] < mv;
      mv = take ? mu[r] : mv;
      k = take ? ri[r] : k;
    }
    Own::template arg<false>(mv, k);
    return mv < Lim<T>::inf();
  }
  // ti = the step at which the first multiplier reaches zero (inf: none), k = its row
  __device__ __forceinline__ void ratio(const int (&st)[RO], const T (&mu)[RO],
                                        const T (&co)[RO], T rm, T sgn, T& ti, int& k) const {
    ti = Lim<T>::inf();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const T dmu = mu_rate(st[r], co[r] * rm, sgn);
      const bool cand = (st[r] == 1 || st[r] == 2) && dmu < T(0);
      const T t = cand ? -mu[r] * fast_rcp(dmu) : Lim<T>::inf();
      const bool take = t < ti;
      ti = take ? t : ti;
      k = take ? ri[r] : k;
    }
    Own::template arg<false>(ti, k);
  }
  // true whenever ratio() would give ti < t2 (RatioFilter); the sentinel is +inf
  __device__ __forceinline__ bool may_block(const int (&st)[RO], const T (&mu)[RO],
                                            const T (&co)[RO], T rm, T sgn, T t2) const {
    return ratio_filter(st, mu, co, rm, sgn, t2) || !ratio_range(t2, Lim<T>::inf());
  }
  // z_p of a new pivot travels with the scan
  template <class Mat>
  __device__ __forceinline__ void publish(const Mat&, const T (&)[RO]) const {}
  __device__ __forceinline__ T pivot_z(int, T zv) const { return zv; }
};

// One fp64 key (Key above; owned rows of a keyed layout).  The code of a row
// is its index mi for an arg-min of non-negative values and cmax = 2^KB-1-mi
// otherwise.  What comes out of a reduction has its low bits clear.
template <class Own>
struct SelKey {
  static constexpr int RO = Own::RO;
  using Mat = typename Own::Mat;
  using K = typename Own::K;
  int mi[RO], cmax[RO];
  double* zs;  // the owners' copy of z in the QP's LDS block
  __device__ __forceinline__ SelKey(const int (&)[RO], const int (&mi_)[RO], double* gb)
      : zs(gb + BoxLds<Mat>::oZ) {
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      mi[r] = mi_[r];
      cmax[r] = int(K::MASK) - mi_[r];
    }
  }
  // A slot that is not free, and a row without a finite bound (NaN: both fmax
  // skip it), pass the sentinel.  viol > tol sees viol to 2^-47 relative; pi
  // is only meaningful when viol > 0.  z_p is not carried (pivot_z).
  __device__ __forceinline__ void scan(const int (&st)[RO], const double (&zr)[RO],
                                       const QBounds<double, RO>& B, double& viol, int& pi,
                                       double&) const {
    double key = -K::big();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const double vl = (B.lo[r] - zr[r]) * B.sl[r];  // NaN for an infinite bound
      const double vu = (zr[r] - B.hi[r]) * B.su[r];
      const double v = fmin(fmax(fmax(vl, vu), -K::big()), K::big());
      key = key_max(key, K::pack((st[r] == 0) ? v : -K::big(), cmax[r]));
    }
    Own::template key_arg<true>(key);
    viol = K::clear(key);
    pi = int(K::MASK) - K::code(key);
  }
  // negative candidates: the larger code is the more negative key
  __device__ __forceinline__ bool release(const int (&st)[RO], const double (&mu)[RO],
                                          double tol, int& k) const {
    double key = K::big();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const bool a = (st[r] == 1 || st[r] == 2) && mu[r] < -tol;
      key = key_min(key, K::pack(a ? fmax(mu[r], -K::big()) : K::big(), cmax[r]));
    }
    Own::template key_arg<false>(key);
    k = int(K::MASK) - K::code(key);
    return K::clear(key) < K::big();
  }
  // ti < t2 sees ti to 2^-47 relative and a partial step has that length.
  // Neither reaches the result: the sweeps do not depend on step lengths, and
  // z and the multipliers come from the exact refresh of the final active set.
  // (fmin maps an infinite or NaN ratio to the sentinel as well; two bit-equal
  // negative ratios, which only rounding in the multipliers produces, resolve
  // to the larger index)
  __device__ __forceinline__ void ratio(const int (&st)[RO], const double (&mu)[RO],
                                        const double (&co)[RO], double rm, double sgn,
                                        double& ti, int& k) const {
    double key = K::big();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const double dmu = mu_rate(st[r], co[r] * rm, sgn);
      const bool cand = (st[r] == 1 || st[r] == 2) && dmu < 0.0;
      const double t = cand ? fmin(-mu[r] * fast_rcp(dmu), K::big()) : K::big();
      key = key_min(key, K::pack(t, mi[r]));
    }
    Own::template key_arg<false>(key);
    ti = K::clear(key);
    k = K::code(key);
  }
  // true whenever ratio() would give ti < t2 (RatioFilter); the sentinel is big()
  __device__ __forceinline__ bool may_block(const int (&st)[RO], const double (&mu)[RO],
                                            const double (&co)[RO], double rm, double sgn,
                                            double t2) const {
    return ratio_filter(st, mu, co, rm, sgn, t2) || !ratio_range(t2, K::big());
  }
  // ratio() and may_block() on the trip's rates dmu[r] = mu_rate(st[r],
  // co[r] * rm, sgn) (RATE_ONCE)
  __device__ __forceinline__ void ratio(const int (&st)[RO], const double (&mu)[RO],
                                        const double (&dmu)[RO], double& ti, int& k) const {
    double key = K::big();
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const bool cand = (st[r] == 1 || st[r] == 2) && dmu[r] < 0.0;
      const double t = cand ? fmin(-mu[r] * fast_rcp(dmu[r]), K::big()) : K::big();
      key = key_min(key, K::pack(t, mi[r]));
    }
    Own::template key_arg<false>(key);
    ti = K::clear(key);
    k = K::code(key);
  }
  __device__ __forceinline__ bool may_block(const int (&st)[RO], const double (&mu)[RO],
                                            const double (&dmu)[RO], double t2) const {
    return ratio_filter(st, mu, dmu, t2) || !ratio_range(t2, K::big());
  }
  // the owners publish their rows of z; a new pivot reads z_p from there
  __device__ __forceinline__ void publish(const Mat& M, const double (&zr)[RO]) const {
#pragma unroll
    for (int r = 0; r < RO; ++r)
      if (Own::has(M, r)) zs[mi[r]] = zr[r];
  }
  __device__ __forceinline__ double pivot_z(int p, double) const { return zs[p]; }
};

// ----------------------------------------------------------- the active set
// One box QP per group / wave; entry: M = -H^{-1}.  Primal and dual quantities
// are tracked incrementally along the steps (z_F, the active multipliers, and
// the multiplier of the bound being added); when every group has settled, one
// exact mat-vec refresh recomputes z and the multipliers and the bounds are
// re-checked, so accumulated drift can never hide a violated bound.
// live = this group holds a real instance.  Returns the status code.
// Own: the row-ownership policy (default: the layout's own, RowOwn<Mat>).
// WARM: st (this lane's rows: 0 free, 1 at lb, 2 at ub, 3 padding) is the
// starting active set and M the matrix swept on its free rows (H swept on F
// equals -H^-1 swept back on the active rows); the active rows whose
// multipliers have the wrong sign are released first (one sweep each), then
// the active set runs as from a cold start.  st is returned either way.
template <bool WARM, class Own_ = void, class Mat, typename T>
__device__ __forceinline__ int gi_box_st(Mat& M, T* gb, const T* fs, const T* lbs,
                                         const T* ubs, int n, int max_iter, T tol, bool live,
                                         T (&zfull)[Mat::RPL], int& iters,
                                         int (&stfull)[Mat::RPL] MPCQP_CLK_PARAM) {
  using Own = std::conditional_t<std::is_void_v<Own_>, RowOwn<Mat>, Own_>;
  static_assert(std::is_same_v<typename Own::Mat, Mat>, "policy of another layout");
  constexpr int BS = Mat::RPL, NC = Mat::NC;  // rows, columns per lane
  // z, the multipliers, the states and the bounds by owned slot (RowOwn)
  constexpr int RO = Own::RO;
  int ri[RO], mi[RO];
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    ri[r] = Own::row(M, r);
    mi[r] = Own::mrow(M, r);
  }
  QBounds<T, RO> B;
  B.load(mi, lbs, ubs);
  const std::conditional_t<Own::KEYED, SelKey<Own>, SelCmp<Own, T>> sel(ri, mi, gb);
  // (replicated: the caller's arrays themselves)
  T zown[Own::OWNED ? RO : 1], mu[RO];
  int stown[Own::OWNED ? RO : 1];
  auto& zr = own_or_full<Own::OWNED>(zown, zfull);
  auto& st = own_or_full<Own::OWNED>(stown, stfull);
  if constexpr (WARM && Own::OWNED) Own::deal(M, stfull, 3, stown);
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    if constexpr (!WARM) st[r] = (Own::has(M, r) && ri[r] < n) ? 0 : 3;
    mu[r] = T(0);
    zr[r] = T(0);
  }
  iters = 0;
  int code = MPCQP_STATUS_OPTIMAL;
  auto refresh = [&]() {
    T w[RO], s[RO];
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const T zA = (st[r] == 1) ? B.lo[r] : ((st[r] == 2) ? B.hi[r] : T(0));
      w[r] = (st[r] == 0) ? fs[mi[r]] : -zA;
      zr[r] = zA;
    }
    Own::matvec(M, w, gb, s);
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      const T g = fs[mi[r]] - s[r];
      zr[r] = (st[r] == 0) ? s[r] : zr[r];
      mu[r] = (st[r] == 1) ? g : ((st[r] == 2) ? -g : T(0));
    }
    sel.publish(M, zr);
  };
  refresh();
  bool active = live;
  if constexpr (WARM) {
    // release wrong-signed multipliers, the most negative first
    bool drop = live;
    while (true) {
      int k = 0;
      const bool found = sel.release(st, mu, tol, k);
      drop = drop && found;
      if (!__any(drop)) break;
      if (drop && ++iters > max_iter) {
        code = MPCQP_STATUS_MAXITER;
        drop = false;
        active = false;
      }
      T kr[BS], kc[NC];
      const T d = M.column(k, gb, kr, kc);
      if (drop && !(d > T(0))) {
        code = MPCQP_STATUS_NOT_CONVEX;
        drop = false;
        active = false;
      }
      if (drop) {
        M.sweep_col(k, T(1), d, kr, kc);
#pragma unroll
        for (int r = 0; r < RO; ++r)
          if (ri[r] == k) st[r] = 0;
      }
      refresh();
    }
  }
  for (int pass = 0; pass < 3; ++pass) {
    bool need_p = true;
    int p = 0, side = 1;
    T tgt = T(0), zp = T(0), gp = T(0);
    // the scan of the trip before (below); a_zv stays unused on a key.  a_lb,
    // a_ub, a_zp (AHEAD): the bounds and z of row a_pi, read behind that scan
    T a_viol = T(0), a_zv = T(0);
    int a_pi = 0;
    [[maybe_unused]] T a_lb = T(0), a_ub = T(0), a_zp = T(0);
    bool have_scan = false;
    while (true) {
      if constexpr (Own::NODRAIN) {
        // every lane takes the read-ahead here: an empty statement, whose
        // operands make the compiler wait for the three reads now and not at
        // the first reuse of their registers, behind the column's publish
        asm volatile("" : : "v"(a_lb), "v"(a_ub), "v"(a_zp));
      }
      if (__any(active && need_p)) {
        T viol, zv = T(0);
        int pi;
        if (have_scan) {
          viol = a_viol;
          pi = a_pi;
          zv = a_zv;
        } else {
          sel.scan(st, zr, B, viol, pi, zv);
        }
        if (active && need_p) {
          if (!(viol > tol)) {
            active = false;  // settled (pending the exact re-check)
          } else {
            p = pi;
            if constexpr (Own::AHEAD) {
              // no LDS wait here but in the first trip of a pass, which has
              // no scan-ahead and reads at the use
              const T lbp = have_scan ? a_lb : lbs[p], ubp = have_scan ? a_ub : ubs[p];
              zp = have_scan ? a_zp : sel.pivot_z(p, zv);
              side = (zp < lbp) ? 1 : 2;
              tgt = (side == 1) ? lbp : ubp;
            } else {
              const T lbp = lbs[p], ubp = ubs[p];
              zp = sel.pivot_z(p, zv);
              side = (zp < lbp) ? 1 : 2;
              tgt = (side == 1) ? lbp : ubp;
            }
            gp = T(0);
            need_p = false;
          }
        }
      }
      MPCQP_PHASE(5);
      if (!__any(active)) break;
      bool stepping = active;
      if (stepping && ++iters > max_iter) {
        code = MPCQP_STATUS_MAXITER;
        active = false;
        stepping = false;
      }
      T c[BS], cc[NC], co[RO];  // c[r] = M_ip by block row, co by owned slot
      const T mpp = Own::column(M, p, gb, c, cc, co);  // M_pp < 0
      const T rm = fast_rcp(mpp);
      const T sgn = (tgt > zp) ? T(1) : T(-1);
      const T t2 = fabs(tgt - zp);
      // The rest of the trip, one body for two paths.  FULL: no group of the
      // wave can take a partial step (the ratio filter, below), so partial is
      // the constant false and with it idx = p, sigma = -1, the sweep column
      // the pivot's; no ratio test, no second column publish.  Per group the
      // arithmetic of a full step is that of the general path, in its order.
      // The sweep itself follows the two paths (one copy: with one in each
      // path M lived in two sets of registers, 169 -> 252 VGPRs at config 2)
      // and takes from them the pivot idx, sigma, the column kr / kcol and
      // d, or (SWEEP_RD) 1 / d, which the full-step path holds already.
      // FULL_SWEEP: the full-step path sweeps inside itself, on c / cc, rm and
      // sigma = -1 as they stand, and only the general path hands over to the
      // sweep below; M still lives in one set of registers (204 -> 233 VGPRs).
      [[maybe_unused]] T s_kr[BS], s_kcol[NC], s_sigma = T(-1), s_d = mpp;
      [[maybe_unused]] int s_idx = p;
      [[maybe_unused]] bool sweeping = false;
      // RATE_ONCE: the multiplier rates of this trip, once for the filter, the
      // ratio test and the step update (outside the filter's short-circuit)
      [[maybe_unused]] T dmu[RO];
      if constexpr (Own::RATE_ONCE) {
#pragma unroll
        for (int r = 0; r < RO; ++r) dmu[r] = mu_rate(st[r], co[r] * rm, sgn);
      }
      // some group of the wave may take a partial step (the ratio filter)
      [[maybe_unused]] bool general = true;
      if constexpr (Own::RATE_ONCE) {
        general = __any(stepping && sel.may_block(st, mu, dmu, t2));
      } else if constexpr (Own::FAST) {
        general = __any(stepping && sel.may_block(st, mu, co, rm, sgn, t2));
      }
      if constexpr (!Own::FAST) {
#define MPCQP_TRIP_FULL false
#include "gi_box_trip.inc"
#undef MPCQP_TRIP_FULL
      } else if (general) {
#define MPCQP_TRIP_FULL false
#include "gi_box_trip.inc"
#undef MPCQP_TRIP_FULL
      } else {
#define MPCQP_TRIP_FULL true
#include "gi_box_trip.inc"
#undef MPCQP_TRIP_FULL
      }
      if constexpr (Own::FAST) {
        if constexpr (Own::SWEEP_FIX) {
          if (sweeping)
            M.template sweep_col<Own::SWEEP_RD, true>(s_idx, s_sigma, s_d, s_kr, s_kcol);
        } else {
          if (sweeping) M.template sweep_col<Own::SWEEP_RD>(s_idx, s_sigma, s_d, s_kr, s_kcol);
        }
      }
      MPCQP_PHASE(7);
    }
    // exact refresh for every group, then re-check the bounds
    refresh();
    T viol, zv = T(0);
    int pi;
    sel.scan(st, zr, B, viol, pi, zv);
    active = live && code == MPCQP_STATUS_OPTIMAL && viol > tol;
    if (!__any(active)) break;
  }
#pragma unroll
  for (int r = 0; r < RO; ++r) {
    zr[r] = fmin(fmax(zr[r], B.lo[r]), B.hi[r]);
  }
  if constexpr (Own::OWNED) {
    Own::gather(M, zown, zfull);
    Own::gather(M, stown, stfull);
  }
  return code;
}

// Cold start: every row free, the states are not returned.
template <class Own = void, class Mat, typename T>
__device__ __forceinline__ int gi_box(Mat& M, T* gb, const T* fs, const T* lbs, const T* ubs,
                                      int n, int max_iter, T tol, bool live,
                                      T (&zr)[Mat::RPL], int& iters MPCQP_CLK_PARAM) {
  int st[Mat::RPL];
  return gi_box_st<false, Own>(M, gb, fs, lbs, ubs, n, max_iter, tol, live, zr, iters,
                               st MPCQP_CLK_ARG);
}

// The one-QP-per-wave kernels: every wave holds a real instance, and the
// phase clock (debug builds) starts here.
template <typename T, int BS>
__device__ __forceinline__ int gi_box_core(Sym2D<T, BS>& M, T* buf, const T* fs, const T* lbs,
                                           const T* ubs, int n, int max_iter, T tol,
                                           T (&zr)[BS], int& iters) {
#ifdef MPCQP_PHASE_TIMING
  PhaseClock mpcqp_clk;
#endif
  return gi_box(M, buf, fs, lbs, ubs, n, max_iter, tol, true, zr, iters MPCQP_CLK_ARG);
}

}  // namespace mpcqp
