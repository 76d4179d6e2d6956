// Instantiations of the pipe step kernel (lmc_step_pipe_kernel.h) for uniform 5 x 5 box blurs -- all of the reference's 5-tap blurs: the L wave's four
// 5-tap passes as plain sums with shared partial sums and no window copies (pipe_body<..., UNI>), the scale c_u c_v applied once.  Kernels of their own name:
//   myula_step_pipe_uni_kernel<10, PXL in {4, 8}, 5>     one team, one launch of 10 dual iterations, aligned rows, one strip
//   myula_step_pipe_uni2_kernel<10, 5>                   the two-team layout (pipe_teams_covered)
// (uni2, not pipe2_uni: the prefix myula_step_pipe2 names the two kernels whose register budget beside the side-stream moment reduction is pinned; this one
// keeps the same budget, tests/test_pipe_uni_resources.py.)  Every sum is defined per pixel: the three kernels give the same bits.
#include "lmc_step_pipe_kernel.h"

namespace lmc {

template <int K, int PXL, int KT>
__global__ __launch_bounds__(64 * ((K + 1) / 2 + 3), PXL == 8 ? 1 : 2) void myula_step_pipe_uni_kernel(const StepArgs A) {
  pipe_body<K, PXL, KT, false, false, true, false, 1, false, false, kTermL2, true>(A);
}

template <int K, int KT>
__global__ __launch_bounds__(128 * ((K + 1) / 2 + 3), 4) void myula_step_pipe_uni2_kernel(const StepArgs A) {
  pipe_body<K, 4, KT, false, false, true, false, 2, false, false, kTermL2, true>(A);
}

template <int PXL>
static hipError_t pipe_uni_launch_one(const StepArgs& a, hipStream_t st) {
  constexpr int K = 10;
  return pipe_launch<myula_step_pipe_uni_kernel<K, PXL, 5>>(pipe_lds_bytes<K, PXL, 5, false>(), dim3(a.C), dim3(pipe_block(K, 1)), a, st);
}

// a.blur.h holds the centred taps (pipe_taps); the caller has checked the coverage (pipe_uni_covered, lmc_step_pipe.hip)
hipError_t pipe_dispatch_uni(const StepArgs& a, int KT, int teams, hipStream_t st) {
  if (a.tv.niter != 10 || KT != 5 || !pipe_lastlane(a.W) || a.W > 512 || a.tv_warm || a.tv_aniso || a.box || a.term != kTermL2 || a.rt_kc) return hipErrorInvalidConfiguration;
  if (teams == 2) return pipe_launch<myula_step_pipe_uni2_kernel<10, 5>>(pipe_teams_lds_bytes<10>(), dim3(a.C), dim3(pipe_block(10, 2)), a, st);
  return a.W > 256 ? pipe_uni_launch_one<8>(a, st) : pipe_uni_launch_one<4>(a, st);
}

}  // namespace lmc
