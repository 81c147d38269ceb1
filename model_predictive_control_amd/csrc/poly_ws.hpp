// poly_ws.hpp -- layout of the shared-factor workspace that mpcqp_poly_setup
// writes and mpcqp_poly_solve / mpcqp_mpc_poly_loop read (solve_poly.hip,
// loop_poly.hip).  Host side only.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mpcqp {

static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// Shared factors; independent of the batch size.
struct PolyWs {
  int64_t oW, oHinv, oUt, oM, oKt, oL, oFlag, total;
};

static inline PolyWs poly_ws(size_t es, int n, int mt, int nx) {
  PolyWs w;
  w.oW = 0;
  w.oHinv = align256(w.oW + (int64_t)n * n * es);
  w.oUt = align256(w.oHinv + (int64_t)n * n * es);
  w.oM = align256(w.oUt + (int64_t)mt * n * es);
  w.oKt = align256(w.oM + (int64_t)mt * (mt + 1) / 2 * es);
  w.oL = align256(w.oKt + (int64_t)nx * n * es);
  w.oFlag = align256(w.oL + (int64_t)mt * nx * es);
  w.total = align256(w.oFlag + 16);
  return w;
}

}  // namespace mpcqp
