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
//
// The counterpart of sym2d.hpp: the layout and its reductions.  The box active
// set that runs on either layout is in gi_box_core.hpp.
#pragma once
#include "sym2d.hpp"

namespace mpcqp {

// Sum over the 4 lanes of a row block (bits 0..1).
template <typename T>
__device__ __forceinline__ T quad_sum(T v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  return v;
}
// value of lane J of the quad (quad_perm broadcast)
template <int J, typename X>
__device__ __forceinline__ X quad_lane(X v) {
  return dpp<J | (J << 2) | (J << 4) | (J << 6)>(v);
}

// Five groups of five 64-bit moves, group i under the lane mask K[i] (a
// ballot, so a subset of the lanes that execute this): D(i, j) = S[j], D(i, j)
// being the lvalue of entry j of group i.  One statement that leaves exec as it
// found it, with no compare and no branch inside (QSym::sweep_col<RD, true>).
// The statement reads exec and must run under the control flow its ballots
// were formed under.  Its operands do not say so: what holds it in place is
// that device-side inline assembly is convergent to the compiler, which
// therefore neither sinks nor hoists it across a divergent branch.  It is not
// volatile (the measured instruction stream is that of the plain statement);
// do not copy it to a place where that property does not hold.
#define MPCQP_MOV5(I)                                                           \
  "s_mov_b64 exec, %[k" #I "]\n\t"                                              \
  "v_mov_b64 %[d" #I "0], %[s0]\n\tv_mov_b64 %[d" #I "1], %[s1]\n\t"            \
  "v_mov_b64 %[d" #I "2], %[s2]\n\tv_mov_b64 %[d" #I "3], %[s3]\n\t"            \
  "v_mov_b64 %[d" #I "4], %[s4]\n\t"
#define MPCQP_MOV5_OUT(I, D)                                                   \
  [d##I##0] "+v"(D(I, 0)), [d##I##1] "+v"(D(I, 1)), [d##I##2] "+v"(D(I, 2)),   \
      [d##I##3] "+v"(D(I, 3)), [d##I##4] "+v"(D(I, 4))
#define MPCQP_MASKED_MOV_5X5(D, K, S)                                          \
  do {                                                                         \
    unsigned long long mpcqp_exec;                                             \
    asm("s_mov_b64 %[t], exec\n\t" MPCQP_MOV5(0) MPCQP_MOV5(1) MPCQP_MOV5(2)    \
            MPCQP_MOV5(3) MPCQP_MOV5(4) "s_mov_b64 exec, %[t]"                 \
        : [t] "=&s"(mpcqp_exec), MPCQP_MOV5_OUT(0, D), MPCQP_MOV5_OUT(1, D),   \
          MPCQP_MOV5_OUT(2, D), MPCQP_MOV5_OUT(3, D), MPCQP_MOV5_OUT(4, D)     \
        : [k0] "s"(K[0]), [k1] "s"(K[1]), [k2] "s"(K[2]), [k3] "s"(K[3]),      \
          [k4] "s"(K[4]), [s0] "v"(S[0]), [s1] "v"(S[1]), [s2] "v"(S[2]),      \
          [s3] "v"(S[3]), [s4] "v"(S[4]));                                     \
  } while (0)

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

  // Arg-max (MAX) / arg-min of (value, index[, payload]) over the 4 row blocks
  // of a group (lanes differing in bits 2..3: row_ror:4, row_ror:8), and over
  // all 16 lanes: the 4 lanes of a row block first, then the row blocks.
  template <bool MAX, typename... P>
  static __device__ __forceinline__ void rows_arg(T& v, int& idx, P&... pay) {
    arg_step<MAX, Dpp<0x124>>(v, idx, pay...);
    arg_step<MAX, Dpp<0x128>>(v, idx, pay...);
  }
  template <bool MAX, typename... P>
  static __device__ __forceinline__ void group_arg(T& v, int& idx, P&... pay) {
    arg_step<MAX, Dpp<0xB1>>(v, idx, pay...);
    arg_step<MAX, Dpp<0x4E>>(v, idx, pay...);
    rows_arg<MAX>(v, idx, pay...);
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

  // Row ownership (RowOwn, gi_box_core.hpp): row r of a row block belongs to lane
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
  // RD: d is already 1 / M_kk = fast_rcp(M_kk), from a caller that holds it (the
  // full-step trip of gi_box_st).  One function with a flag and not a second
  // one that the first forwards to: forwarding changes the instruction streams
  // of five fp32 BS = 2 kernels that never pass RD.
  // FIX: the same three candidates reach m[r][c] another way.  Every entry
  // takes gen; then the lanes that hold column k overwrite it with scol and the
  // lanes that hold row k overwrite that with srow (row k wins at (k, k), as in
  // the nested select): BS 64-bit moves under the lane mask of one compare
  // instead of two 32-bit selects per entry and level.  Same operands, same
  // operations, same bits.  The moves are one inline-assembly statement per
  // level that sets exec from the masks (MPCQP_MASKED_MOV_5X5): written as
  // assignments under `if` the compiler selects again, and with only the move
  // in assembly it builds ten regions of compare, saveexec and branch, which
  // measured slower than the selects.
  template <bool RD = false, bool FIX = false>
  __device__ __forceinline__ void sweep_col(int k, T sigma, T d, const T (&colr)[BS],
                                            const T (&colc)[BS]) {
    const T rd = RD ? d : fast_rcp(d);
    T a[BS], scol[BS], srow[BS];
    bool jk[BS];
    if constexpr (FIX) {
      static_assert(BS == 5 && sizeof(T) == 8, "the masked moves are written for 5 x 5 fp64");
      unsigned long long ikm[BS], jkm[BS];
#pragma unroll
      for (int r = 0; r < BS; ++r) {
        a[r] = colr[r] * rd;
        scol[r] = sigma * a[r];
        ikm[r] = __builtin_amdgcn_ballot_w64(bi * BS + r == k);
#pragma unroll
        for (int c = 0; c < BS; ++c) m[r][c] = fma(-a[r], colc[c], m[r][c]);
      }
#pragma unroll
      for (int c = 0; c < BS; ++c) {
        jk[c] = (bj * BS + c == k);
        jkm[c] = __builtin_amdgcn_ballot_w64(jk[c]);
        srow[c] = jk[c] ? -rd : sigma * colc[c] * rd;
      }
#define MPCQP_COL(I, J) m[J][I]
#define MPCQP_ROW(I, J) m[I][J]
      MPCQP_MASKED_MOV_5X5(MPCQP_COL, jkm, scol);
      MPCQP_MASKED_MOV_5X5(MPCQP_ROW, ikm, srow);
#undef MPCQP_COL
#undef MPCQP_ROW
    } else {
      bool ik[BS];
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

}  // namespace mpcqp
