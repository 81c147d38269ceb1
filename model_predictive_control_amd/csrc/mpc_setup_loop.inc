// mpc_setup_loop.inc -- the setup loop of mpc_group_kernel (quad_box.hip) for
// one combination of the launch flags (MPCQP_STAGE_TV, MPCQP_STAGE_HC as
// literals).  PAIRS (QMpcUniform::level == 2): two stages per trip, so that
// what one stage hands to the next (Psi, P, x-bar, the read-ahead) is not
// copied round the loop and the second stage's independent work fills the
// first one's waits, and the stage that an odd N leaves over.  Written out:
// the unroller turns "#pragma unroll 2" down for this loop.
{
  if constexpr (PAIRS) {
    for (int t2 = 0; t2 + 1 < N; t2 += 2) {
      {
        const int t = t2;
#include "mpc_setup_stage.inc"
      }
      {
        const int t = t2 + 1;
#include "mpc_setup_stage.inc"
      }
    }
    if (N & 1) {
      const int t = N - 1;
#include "mpc_setup_stage.inc"
    }
  } else {
    for (int t = 0; t < N; ++t)
#include "mpc_setup_stage.inc"
  }
}
