// quad.hpp -- four QPs per wavefront, one per 16-lane DPP row ("group").
//
// Lane l: group g = l >> 4, and inside the group q = l & 15, bi = q >> 2,
// bj = q & 3.  A symmetric n x n matrix (n <= 4*BS) of group g is held as a
// 4 x 4 grid of BS x BS register blocks over the group's 16 lanes.  All
// per-QP scalars (pivot index, step lengths, ...) are group-uniform VGPR
// values; every reduction stays inside a DPP row (quad_perm for the 4 lanes
// of a row block, row_ror:4/8 across row blocks), so four independent QPs
// share each instruction and no cross-row traffic (bpermute) is needed.
//
// Compared with one QP per wavefront (sym2d.hpp) the per-iteration bookkeeping
// -- reductions, LDS publishes, waits, scalar control -- is paid once for four
// problems, which is what bounds the solve at the config-2 sizes (the SIMDs
// are instruction-issue bound, see profiles/).
#pragma once
#include "sym2d.hpp"

#ifndef MPCQP_SCAN_AHEAD
#define MPCQP_SCAN_AHEAD 1
#endif

namespace mpcqp {

// Max over the 4 row blocks of a group (lanes differing in bits 2..3),
// carrying an index and one payload value; ties to the smaller index.
template <typename T>
__device__ __forceinline__ void group_argmax(T& v, int& idx, T& pay) {
  {
    const T ov = dpp<0x124>(v);  // row_ror:4
    const int oi = dpp<0x124>(idx);
    const T op = dpp<0x124>(pay);
    const bool take = (ov > v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
    pay = take ? op : pay;
  }
  {
    const T ov = dpp<0x128>(v);  // row_ror:8
    const int oi = dpp<0x128>(idx);
    const T op = dpp<0x128>(pay);
    const bool take = (ov > v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
    pay = take ? op : pay;
  }
}

template <typename T>
__device__ __forceinline__ void group_argmin(T& v, int& idx) {
  {
    const T ov = dpp<0x124>(v);
    const int oi = dpp<0x124>(idx);
    const bool take = (ov < v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
  {
    const T ov = dpp<0x128>(v);
    const int oi = dpp<0x128>(idx);
    const bool take = (ov < v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
}

// Sum over the 4 lanes of a row block (bits 0..1).
template <typename T>
__device__ __forceinline__ T quad_sum(T v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  return v;
}

template <typename T, int BS>
struct QSym {
  static constexpr int NMAX = 4 * BS;
  static constexpr int NV = NMAX;  // row-indexed vectors
  static constexpr int NC = BS;    // columns per lane
  static constexpr int RPL = BS;   // rows per lane
  static constexpr int CBUF = NMAX * BS;  // column-publish tile (per group)
  static constexpr int BUF = CBUF + NMAX;  // + mat-vec vector
  T m[BS][BS];
  int bi, bj;

  __device__ __forceinline__ void init(int lane) {
    const int q = lane & 15;
    bi = q >> 2;
    bj = q & 3;
  }

  // From a dense row-major n x n matrix (leading dim ld) in LDS, symmetrised.
  __device__ __forceinline__ void load_dense_sym(const T* D, int ld, int n) {
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        const int i = bi * BS + r, j = bj * BS + c;
        m[r][c] = (i < n && j < n) ? T(0.5) * (D[i * ld + j] + D[j * ld + i]) : T(0);
      }
  }

  __device__ __forceinline__ void load_packed(const T* Ps, int n, bool& nonfinite) {
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        const int i = bi * BS + r, j = bj * BS + c;
        T v = T(0);
        if (i < n && j < n) {
          const int idx = (j <= i) ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;
          v = Ps[idx];
          nonfinite |= !finite(v);
        }
        m[r][c] = v;
      }
  }

  // Row ownership (RowOwn below): row r of a row block belongs to lane
  // bj = r mod 4, so a lane owns RO rows, slot s holding row 4 s + bj.
  static constexpr int RO = (BS + 3) / 4;
  __device__ __forceinline__ int own_row(int s) const { return 4 * s + bj; }
  __device__ __forceinline__ bool owns(int s) const { return own_row(s) < BS; }
  // the same for addressing: a slot without a row reads the block's last row
  __device__ __forceinline__ int own_mrow(int s) const {
    return own_row(s) < BS ? own_row(s) : BS - 1;
  }

  // Column k (group-uniform) through the group's LDS tile; returns M_kk.
  // (the owners' reads below are dead here: their results are never used,
  // and the compiler drops the loads -- same ds_read count as before)
  __device__ __forceinline__ T column(int k, T* gb, T (&colr)[BS], T (&colc)[BS]) {
    T unused[RO];
    return column(k, gb, colr, colc, unused);
  }
  // The same, and cown[s] = M[row of slot s][k] for the rows this lane owns.
  __device__ __forceinline__ T column(int k, T* gb, T (&colr)[BS], T (&colc)[BS],
                                      T (&cown)[RO]) {
    const int kb = k / BS, kc = k - kb * BS;
    if (bj == kb) {
#pragma unroll
      for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c) gb[(bi * BS + r) * BS + c] = m[r][c];
    }
    lds_exchange();
#pragma unroll
    for (int r = 0; r < BS; ++r) colr[r] = gb[(bi * BS + r) * BS + kc];
#pragma unroll
    for (int c = 0; c < BS; ++c) colc[c] = gb[(bj * BS + c) * BS + kc];
    // (a static select out of colr instead of these reads measured the same)
#pragma unroll
    for (int s = 0; s < RO; ++s) cown[s] = gb[(bi * BS + own_mrow(s)) * BS + kc];
    const T d = gb[k * BS + kc];
    lds_exchange();
    return d;
  }

  // Goodnight sweep (sigma = +1) / reverse sweep (sigma = -1) on pivot k with
  // its column already fetched:  M_ij - M_ik M_kj / d  off row/column k,
  // sigma M_kj / d on row k, sigma M_ik / d on column k, -1/d at (k, k).
  // Row/column k are selected, not produced by cancellation (their relative
  // error would otherwise grow like eps * |d|).
  __device__ __forceinline__ void sweep_col(int k, T sigma, T d, const T (&colr)[BS],
                                            const T (&colc)[BS]) {
    const T rd = fast_rcp(d);
    T a[BS], scol[BS], srow[BS];
    bool ik[BS], jk[BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      a[r] = colr[r] * rd;
      scol[r] = sigma * a[r];
      ik[r] = (bi * BS + r == k);
    }
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      jk[c] = (bj * BS + c == k);
      srow[c] = jk[c] ? -rd : sigma * colc[c] * rd;
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        const T gen = fma(-a[r], colc[c], m[r][c]);
        m[r][c] = ik[r] ? srow[c] : (jk[c] ? scol[r] : gen);
      }
  }

  __device__ __forceinline__ T sweep(int k, T sigma, T* gb) {
    T colr[BS], colc[BS];
    const T d = column(k, gb, colr, colc);
    sweep_col(k, sigma, d, colr, colc);
    return d;
  }

  // out[r] = sum_j M[i][j] w[j] (w in the group's row-block layout).
  __device__ __forceinline__ void matvec(const T (&w)[BS], T* gb, T (&out)[BS]) {
    T* wb = gb + CBUF;
    if (bj == 0) {
#pragma unroll
      for (int r = 0; r < BS; ++r) wb[bi * BS + r] = w[r];
    }
    lds_exchange();
    T wc[BS];
#pragma unroll
    for (int c = 0; c < BS; ++c) wc[c] = wb[bj * BS + c];
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      T s = T(0);
#pragma unroll
      for (int c = 0; c < BS; ++c) s = fma(m[r][c], wc[c], s);
      out[r] = quad_sum(s);
    }
    lds_exchange();
  }

  // The same on owned rows: the owners store w, every lane of a row block
  // forms the block's BS sums (same products, same quad_sum) and keeps its own.
  __device__ __forceinline__ void matvec_own(const T (&w)[RO], T* gb, T (&out)[RO]) {
    T* wb = gb + CBUF;
#pragma unroll
    for (int s = 0; s < RO; ++s)
      if (owns(s)) wb[bi * BS + own_row(s)] = w[s];
    lds_exchange();
    T wc[BS];
#pragma unroll
    for (int c = 0; c < BS; ++c) wc[c] = wb[bj * BS + c];
#pragma unroll
    for (int s = 0; s < RO; ++s) out[s] = T(0);
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      T s = T(0);
#pragma unroll
      for (int c = 0; c < BS; ++c) s = fma(m[r][c], wc[c], s);
      s = quad_sum(s);
      out[r / 4] = (bj == r % 4) ? s : out[r / 4];
    }
    lds_exchange();
  }
};

// Keyed reductions (below, next to dpp_argmax): which layouts reduce the scan,
// the ratio test and the warm-start release scan on one fp64 key instead of
// a (value, index, payload) triple.  fp64 only: in fp32 the index bits would
// make values within 2^-18 relative compare equal.
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

// Per-group LDS block for the box active set: [Mat::BUF | f | lb | ub | z],
// the vectors indexed by (padded) row; oBuf = 0, so the tile pointer gb is
// the block's base.  z (keyed layouts only, otherwise empty) is the owners'
// copy of the primal iterate, from which a new pivot reads z_p.
template <class Mat>
struct GBoxLds {
  static constexpr int NMAX = Mat::NMAX;
  static constexpr int NV = Mat::NV;
  static constexpr int oBuf = 0;
  static constexpr int oF = Mat::BUF;
  static constexpr int oLb = oF + NV;
  static constexpr int oUb = oLb + NV;
  static constexpr int oZ = oUb + NV;
  static constexpr int size = oZ + (QKeyed<Mat>::v ? NV : 0);
};
template <typename T, int BS>
using QBoxLds = GBoxLds<QSym<T, BS>>;

// Relative-violation scale of a bound: 1/(1+|b|) for a finite bound, NaN for
// an infinite one (a NaN violation never wins the arg-max and fmax skips it),
// so the per-iteration scan multiplies instead of dividing.
template <typename T>
__device__ __forceinline__ T bound_scale(T bnd) {
  return finite(bnd) ? T(1) / (T(1) + fabs(bnd)) : __builtin_nan("");
}

// Goldfarb-Idnani dual active set for one box QP per group / wave (see gi_box_core.hpp
// for the method); entry: M = -H^{-1}.  Primal and dual quantities are tracked
// incrementally along the steps (z_F, the active multipliers, and the
// multiplier of the bound being added); when every group has settled, one
// exact mat-vec refresh recomputes z and the multipliers and the bounds are
// re-checked, so accumulated drift can never hide a violated bound.
// live = this group holds a real instance.  Returns the status code.
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

// Reductions over the rows of one QP, per layout: four QPs per wave (DPP
// rows of 16 lanes) or one QP per wave (8 row blocks).
template <typename T, int BS>
__device__ __forceinline__ void rows_argmax(const QSym<T, BS>&, T& v, int& idx, T& pay) {
  group_argmax(v, idx, pay);
}
template <typename T, int BS>
__device__ __forceinline__ void rows_argmin(const QSym<T, BS>&, T& v, int& idx) {
  group_argmin(v, idx);
}
template <typename T, int BS>
__device__ __forceinline__ void rows_argmax(const Sym2D<T, BS>&, T& v, int& idx, T& pay) {
  blocks_argmax(v, idx, pay);
}
template <typename T, int BS>
__device__ __forceinline__ void rows_argmin(const Sym2D<T, BS>&, T& v, int& idx) {
  blocks_argmin(v, idx);
}


// One step of an arg-max / arg-min over DPP pattern CTRL; the same total
// order as group_argmax / group_argmin (value, then the smaller index).
template <int CTRL, typename T>
__device__ __forceinline__ void dpp_argmax(T& v, int& idx, T& pay) {
  const T ov = dpp<CTRL>(v);
  const int oi = dpp<CTRL>(idx);
  const T op = dpp<CTRL>(pay);
  const bool take = (ov > v) || (ov == v && oi < idx);
  v = take ? ov : v;
  idx = take ? oi : idx;
  pay = take ? op : pay;
}
template <int CTRL, typename T>
__device__ __forceinline__ void dpp_argmin(T& v, int& idx) {
  const T ov = dpp<CTRL>(v);
  const int oi = dpp<CTRL>(idx);
  const bool take = (ov < v) || (ov == v && oi < idx);
  v = take ? ov : v;
  idx = take ? oi : idx;
}
// value of lane J of the quad (quad_perm broadcast)
template <int J, typename X>
__device__ __forceinline__ X quad_lane(X v) {
  return dpp<J | (J << 2) | (J << 4) | (J << 6)>(v);
}

// Keyed reductions.  The order of the arg-reductions above (value, then the
// smaller index) fits in one fp64 key: the low KB = ceil(log2 NMAX) mantissa
// bits of the value are replaced by a code of the row index, and a reduction
// step is two DPP moves and one v_max_f64 / v_min_f64 instead of the moves,
// compares and selects of a (value, index, payload) triple.
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
template <int CTRL>
__device__ __forceinline__ void dpp_keymax(double& key) {
  key = key_max(key, dpp<CTRL>(key));
}
template <int CTRL>
__device__ __forceinline__ void dpp_keymin(double& key) {
  key = key_min(key, dpp<CTRL>(key));
}

// Row ownership: which lanes hold the row-indexed vectors of the box active
// set (z, the multipliers, the states, the bounds and their scales).
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

// KEY: keyed reductions where the layout has them (QKeyed); a kernel passes
// false to keep one instantiation on the compare-and-select reductions.
template <class Mat, bool OWN_ROWS = QRowOwned<Mat>::v, bool KEY = true>
struct RowOwn {  // replicated
  static constexpr bool OWNED = false;
  static constexpr bool KEYED = false;
  static constexpr int BS = Mat::RPL;
  static constexpr int RO = BS;
  // slot s holds a row; its matrix row, to compare with a pivot (-1: none)
  // and to address LDS
  static __device__ __forceinline__ bool has(const Mat&, int) { return true; }
  static __device__ __forceinline__ int row(const Mat& M, int s) { return M.bi * BS + s; }
  static __device__ __forceinline__ int mrow(const Mat& M, int s) { return M.bi * BS + s; }
  template <typename T>
  static __device__ __forceinline__ void argmax(const Mat& M, T& v, int& idx, T& pay) {
    rows_argmax(M, v, idx, pay);
  }
  template <typename T>
  static __device__ __forceinline__ void argmin(const Mat& M, T& v, int& idx) {
    rows_argmin(M, v, idx);
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

template <class Mat, bool KEY>
struct RowOwn<Mat, true, KEY> {  // owned (QSym)
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
  template <typename T>
  static __device__ __forceinline__ void argmax(const Mat&, T& v, int& idx, T& pay) {
    dpp_argmax<0xB1>(v, idx, pay);
    dpp_argmax<0x4E>(v, idx, pay);
    group_argmax(v, idx, pay);
  }
  template <typename T>
  static __device__ __forceinline__ void argmin(const Mat&, T& v, int& idx) {
    dpp_argmin<0xB1>(v, idx);
    dpp_argmin<0x4E>(v, idx);
    group_argmin(v, idx);
  }
  // the same reductions on one key (QKeyed)
  static constexpr bool KEYED = KEY && QKeyed<Mat>::v;
  using K = Key<key_bits(Mat::NMAX)>;
  static __device__ __forceinline__ void keymax(double& key) {
    dpp_keymax<0xB1>(key);
    dpp_keymax<0x4E>(key);
    dpp_keymax<0x124>(key);
    dpp_keymax<0x128>(key);
  }
  static __device__ __forceinline__ void keymin(double& key) {
    dpp_keymin<0xB1>(key);
    dpp_keymin<0x4E>(key);
    dpp_keymin<0x124>(key);
    dpp_keymin<0x128>(key);
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

// The most violated free row of a QP: ri = the rows of this lane's slots.
// zv: its z.
template <typename T, class Own, class Mat>
__device__ __forceinline__ void qscan(const Mat& M, const int (&ri)[Own::RO],
                                      const int (&st)[Own::RO], const T (&zr)[Own::RO],
                                      const QBounds<T, Own::RO>& B, T& viol, int& pi, T& zv) {
  viol = -Lim<T>::inf();
  pi = 0;
  zv = T(0);
#pragma unroll
  for (int r = 0; r < Own::RO; ++r) {
    const T vl = (B.lo[r] - zr[r]) * B.sl[r];  // NaN for an infinite bound
    const T vu = (zr[r] - B.hi[r]) * B.su[r];
    const T v = (st[r] == 0) ? fmax(vl, vu) : -Lim<T>::inf();
    const bool take = v > viol;
    viol = take ? v : viol;
    pi = take ? ri[r] : pi;
    zv = take ? zr[r] : zv;
  }
  Own::argmax(M, viol, pi, zv);
}

// The same on one key (Own::KEYED); cmax = 2^KB-1-row of this lane's slots.
// A slot that is not free, and a row without a finite bound (NaN: both fmax
// skip it), pass the sentinel.  viol comes back with its low bits clear, so
// viol > tol sees it to 2^-47 relative; pi is only meaningful when viol > 0.
// z_p is not carried: a new pivot reads it from the owners' LDS copy.
template <class Own>
__device__ __forceinline__ void qscan_key(const int (&cmax)[Own::RO], const int (&st)[Own::RO],
                                          const double (&zr)[Own::RO],
                                          const QBounds<double, Own::RO>& B, double& viol,
                                          int& pi) {
  using K = typename Own::K;
  double key = -K::big();
#pragma unroll
  for (int r = 0; r < Own::RO; ++r) {
    const double vl = (B.lo[r] - zr[r]) * B.sl[r];  // NaN for an infinite bound
    const double vu = (zr[r] - B.hi[r]) * B.su[r];
    const double v = fmin(fmax(fmax(vl, vu), -K::big()), K::big());
    key = key_max(key, K::pack((st[r] == 0) ? v : -K::big(), cmax[r]));
  }
  Own::keymax(key);
  viol = K::clear(key);
  pi = int(K::MASK) - K::code(key);
}


// WARM: st (this lane's rows: 0 free, 1 at lb, 2 at ub, 3 padding) is the
// starting active set and M the matrix swept on its free rows (H swept on F
// equals -H^-1 swept back on the active rows); the active rows whose
// multipliers have the wrong sign are released first (one sweep each), then
// the active set runs as from a cold start.  st is returned either way.
template <typename T, int BS, bool WARM, class Mat, class Own = RowOwn<Mat>>
__device__ __forceinline__ int gi_box_st(Mat& M, T* gb, const T* fs, const T* lbs,
                                         const T* ubs, int n, int max_iter, T tol, bool live,
                                         T (&zfull)[BS], int& iters,
                                         int (&stfull)[BS] MPCQP_CLK_PARAM) {
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
  // keyed reductions (Own::KEYED): the index codes of this lane's slots, and
  // the owners' copy of z in the group's LDS block (GBoxLds::oZ)
  constexpr bool KEYED = Own::KEYED;
  [[maybe_unused]] int cmin[RO], cmax[RO];
  [[maybe_unused]] T* zs = gb + GBoxLds<Mat>::oZ;
  if constexpr (KEYED) {
#pragma unroll
    for (int r = 0; r < RO; ++r) {
      cmin[r] = mi[r];
      cmax[r] = int(Own::K::MASK) - mi[r];
    }
  }
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
    if constexpr (KEYED) {
#pragma unroll
      for (int r = 0; r < RO; ++r)
        if (Own::has(M, r)) zs[mi[r]] = zr[r];
    }
  };
  refresh();
  bool active = live;
  if constexpr (WARM) {
    // release wrong-signed multipliers, the most negative first
    bool drop = live;
    while (true) {
      T mv = Lim<T>::inf();
      int k = 0;
      if constexpr (KEYED) {
        // negative candidates: the larger code is the more negative key
        using K = typename Own::K;
        T key = K::big();
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const bool a = (st[r] == 1 || st[r] == 2) && mu[r] < -tol;
          key = key_min(key, K::pack(a ? fmax(mu[r], -K::big()) : K::big(), cmax[r]));
        }
        Own::keymin(key);
        mv = K::clear(key);
        k = int(K::MASK) - K::code(key);
        drop = drop && mv < K::big();
      } else {
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const bool a = (st[r] == 1 || st[r] == 2) && mu[r] < -tol;
          const bool take = a && mu[r] < mv;
          mv = take ? mu[r] : mv;
          k = take ? ri[r] : k;
        }
        Own::argmin(M, mv, k);
        drop = drop && mv < Lim<T>::inf();
      }
      if (!__any(drop)) break;
      if (drop && ++iters > max_iter) {
        code = MPCQP_STATUS_MAXITER;
        drop = false;
        active = false;
      }
      T kr[BS], kc[Mat::NC];
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
#if MPCQP_SCAN_AHEAD
    T a_viol = T(0), a_zv = T(0);
    int a_pi = 0;
    bool have_scan = false;
#endif
    while (true) {
      if (__any(active && need_p)) {
        T viol, zv = T(0);  // (keyed: z_p comes from LDS, zv stays unused)
        int pi;
#if MPCQP_SCAN_AHEAD
        if (have_scan) {
          viol = a_viol;
          pi = a_pi;
          zv = a_zv;
        } else {
          if constexpr (KEYED) qscan_key<Own>(cmax, st, zr, B, viol, pi);
          else qscan<T, Own>(M, ri, st, zr, B, viol, pi, zv);
        }
#else
        if constexpr (KEYED) qscan_key<Own>(cmax, st, zr, B, viol, pi);
        else qscan<T, Own>(M, ri, st, zr, B, viol, pi, zv);
#endif
        if (active && need_p) {
          if (!(viol > tol)) {
            active = false;  // settled (pending the exact re-check)
          } else {
            p = pi;
            if constexpr (!KEYED) zp = zv;
            const T lbp = lbs[p], ubp = ubs[p];
            if constexpr (KEYED) zp = zs[p];
            side = (zp < lbp) ? 1 : 2;
            tgt = (side == 1) ? lbp : ubp;
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
      constexpr int NC = Mat::NC;  // columns per lane
      T c[BS], cc[NC], co[RO];  // c[r] = M_ip by block row, co by owned slot
      const T mpp = Own::column(M, p, gb, c, cc, co);  // M_pp < 0
      const T rm = fast_rcp(mpp);
      const T sgn = (tgt > zp) ? T(1) : T(-1);
      const T t2 = fabs(tgt - zp);
      T ti = Lim<T>::inf();
      int k = 0;
      if constexpr (KEYED) {
        // ti comes back with its low bits clear: ti < t2 sees it to 2^-47
        // relative and a partial step has that length.  Neither reaches the
        // result: the sweeps do not depend on step lengths, and z and the
        // multipliers come from the exact refresh() of the final active set.
        // (fmin maps an infinite or NaN ratio to the sentinel as well; two
        // bit-equal negative ratios, which only rounding in the multipliers
        // produces, resolve to the larger index)
        using K = typename Own::K;
        T key = K::big();
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const T cs = co[r] * rm;
          const T dmu = ((st[r] == 1) ? -cs : ((st[r] == 2) ? cs : T(0))) * sgn;
          const bool cand = (st[r] == 1 || st[r] == 2) && dmu < T(0);
          const T t = cand ? fmin(-mu[r] * fast_rcp(dmu), K::big()) : K::big();
          key = key_min(key, K::pack(t, cmin[r]));
        }
        Own::keymin(key);
        ti = K::clear(key);
        k = K::code(key);
      } else {
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const T cs = co[r] * rm;  // dz per unit move of z_p (c stays raw for the sweep)
          const T dmu = ((st[r] == 1) ? -cs : ((st[r] == 2) ? cs : T(0))) * sgn;
          const bool cand = (st[r] == 1 || st[r] == 2) && dmu < T(0);
          const T t = cand ? -mu[r] * fast_rcp(dmu) : Lim<T>::inf();
          const bool take = t < ti;
          ti = take ? t : ti;
          k = take ? ri[r] : k;
        }
        Own::argmin(M, ti, k);
      }
      const bool partial = ti < t2;
      const T s_eff = stepping ? (partial ? ti : t2) : T(0);
#pragma unroll
      for (int r = 0; r < RO; ++r) {
        const T cs = co[r] * rm;
        const T dmu = ((st[r] == 1) ? -cs : ((st[r] == 2) ? cs : T(0))) * sgn;
        zr[r] = (st[r] == 0) ? fma(sgn * s_eff, cs, zr[r]) : zr[r];
        mu[r] = fma(s_eff, dmu, mu[r]);
      }
      gp = fma(-sgn * s_eff, rm, gp);  // d g_p / d z_p = -1 / M_pp
      zp = fma(sgn, s_eff, zp);
      MPCQP_PHASE(6);
      // the index whose state changes: k joins F (partial) or p leaves it (full)
      const int idx = partial ? k : p;
      const T sigma = partial ? T(1) : T(-1);
      // full steps sweep on p, whose column is still in registers: publish
      // again only when some group of the wave drops a bound
      T kr[BS], kcol[NC];
      T d = mpp;
      if (__any(stepping && partial)) {
        d = M.column(idx, gb, kr, kcol);
      } else {
#pragma unroll
        for (int r = 0; r < BS; ++r) kr[r] = c[r];
#pragma unroll
        for (int r = 0; r < NC; ++r) kcol[r] = cc[r];
      }
      const bool bad = stepping && (partial ? !(d > T(0)) : !(d < T(0)));
#if MPCQP_SCAN_AHEAD
      // the state changes first, then the next pivot's scan: it reads only z
      // and the states, so its arg-max chain runs ahead of (and can overlap)
      // the sweep; used when the step was full (need_p)
      if (stepping && !bad) {
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const int i = ri[r];
          if (partial && i == k) {
            st[r] = 0;
            mu[r] = T(0);
          }
          if (!partial && i == p) {
            st[r] = side;
            zr[r] = tgt;
            mu[r] = (side == 1) ? gp : -gp;
          }
        }
        need_p = !partial;
      }
      if (bad) {
        code = MPCQP_STATUS_NOT_CONVEX;
        active = false;
      }
      if constexpr (KEYED) {
#pragma unroll
        for (int r = 0; r < RO; ++r)
          if (Own::has(M, r)) zs[mi[r]] = zr[r];
      }
      if constexpr (KEYED) qscan_key<Own>(cmax, st, zr, B, a_viol, a_pi);
      else qscan<T, Own>(M, ri, st, zr, B, a_viol, a_pi, a_zv);
      have_scan = true;
      if (stepping && !bad) M.sweep_col(idx, sigma, d, kr, kcol);
      MPCQP_PHASE(7);
#else
      if (stepping && !bad) {
        M.sweep_col(idx, sigma, d, kr, kcol);
#pragma unroll
        for (int r = 0; r < RO; ++r) {
          const int i = ri[r];
          if (partial && i == k) {
            st[r] = 0;
            mu[r] = T(0);
          }
          if (!partial && i == p) {
            st[r] = side;
            zr[r] = tgt;
            mu[r] = (side == 1) ? gp : -gp;
          }
        }
        need_p = !partial;
      }
      if constexpr (KEYED) {
#pragma unroll
        for (int r = 0; r < RO; ++r)
          if (Own::has(M, r)) zs[mi[r]] = zr[r];
      }
      MPCQP_PHASE(7);
      if (bad) {
        code = MPCQP_STATUS_NOT_CONVEX;
        active = false;
      }
#endif
    }
    // exact refresh for every group, then re-check the bounds
    refresh();
    T viol, zv = T(0);
    int pi;
    if constexpr (KEYED) qscan_key<Own>(cmax, st, zr, B, viol, pi);
    else qscan<T, Own>(M, ri, st, zr, B, viol, pi, zv);
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

template <typename T, int BS, class Mat, class Own = RowOwn<Mat>>
__device__ __forceinline__ int gi_box(Mat& M, T* gb, const T* fs, const T* lbs,
                                           const T* ubs, int n, int max_iter, T tol, bool live,
                                           T (&zr)[BS], int& iters MPCQP_CLK_PARAM) {
  int st[BS];
  return gi_box_st<T, BS, false, Mat, Own>(M, gb, fs, lbs, ubs, n, max_iter, tol, live, zr, iters,
                                 st MPCQP_CLK_ARG);
}

}  // namespace mpcqp
