// api.cpp -- ABI version, thread-local error text, HIP error mapping.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/mpcqp.h"
#include "quad_api.hpp"

namespace mpcqp {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* where) {
  set_error("%s: HIP error %d (%s)", where, (int)e, hipGetErrorString(e));
  return MPCQP_EHIP;
}

}  // namespace mpcqp

extern "C" int mpcqp_abi_version(void) { return MPCQP_ABI_VERSION; }

extern "C" const char* mpcqp_last_error(void) { return mpcqp::g_err; }

// Adjoint of the box QP (kernel in box_vjp.hip): the argument checks, all
// before any device work.
namespace mpcqp {
template <typename T>
static int box_vjp_t(int batch, int n, const void* H, int64_t sH, const void* z, const void* lb,
                     int64_t slb, const void* ub, int64_t sub, const int32_t* status,
                     const void* gz, void* gf, void* glb, void* gub, void* gH, int32_t* vstatus,
                     hipStream_t st) {
  BoxVjpArgs<T> a{batch, n, (const T*)H, sH, (const T*)z, (const T*)lb, slb, (const T*)ub, sub,
                  status, (const T*)gz, (T*)gf, (T*)glb, (T*)gub, (T*)gH, vstatus};
  return solve_box_vjp_quad<T>(a, st);
}
}  // namespace mpcqp

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
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MPCQP_F64)
    return box_vjp_t<double>(batch, n, H, strideH, z, lb, strideLb, ub, strideUb, status, gz, gf,
                             glb, gub, gH, vstatus, st);
  return box_vjp_t<float>(batch, n, H, strideH, z, lb, strideLb, ub, strideUb, status, gz, gf, glb,
                          gub, gH, vstatus, st);
}
