// poly_prep.hpp -- the launcher of poly_affine_prep_kernel (loop_poly.hip) for
// the other translation units that need its products (poly_vjp.hip).  Host
// side only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcqp {

// zg = -Hinv g (R x n) and sg = -Ut g (R x mt) for the R rows of g, with Hinv
// (n x n) and Ut (mt x n) of the mpcqp_poly_setup workspace; mt <= 64.
// Enqueues one launch on st.  `who` names the entry point in an error message.
int launch_poly_affine_prep(const char* who, int dtype, const void* g, int64_t R, int n, int mt,
                            const void* Hinv, const void* Ut, void* zg, void* sg,
                            hipStream_t st);

}  // namespace mpcqp
