// Instantiations of the pipe step kernel (lmc_step_pipe_kernel.h) for the box-constrained isotropic TV prior, g(x) = sigma TV(x) + the indicator of
// [box_lo, box_hi]: Beck and Teboulle's fast gradient projection with constraints -- the same pipeline with the primal iterate projected onto the box
// in every stage and in the combine wave (pipe_stage<..., BOX>), which is the prox MYULA needs for the constrained sampler of Durmus, Moulines and
// Pereyra.  Kernels of their own name, so that the argument lists of myula_step_pipe_kernel / myula_step_pipe2_kernel and of the anisotropic kernels
// stay as they are:
//   myula_step_pipe_box_kernel<K = 10, PXL in {4, 8}, KT in {0, 5, 7}, CHAIN, AL>     one launch of 10 dual iterations, or one link of a chain
//   myula_step_pipe_box2_kernel<10, 5>                                                 the two-team layout (pipe_teams_covered)
// (box2, not pipe2_box: the prefix myula_step_pipe2 names the two kernels whose register budget beside the side-stream moment reduction is pinned.)
// No early exit (RT), no warm dual, and no anisotropic form (that prior takes its box in the tile kernel).  The bounds are StepArgs::box_lo / box_hi.
#include "lmc_step_pipe_kernel.h"

namespace lmc {

template <int K, int PXL, int KT, bool CHAIN, bool AL>
__global__ __launch_bounds__(64 * ((K + 1) / 2 + 3), (PXL == 8 || CHAIN) ? 1 : 2) void myula_step_pipe_box_kernel(const StepArgs A) {
  pipe_body<K, PXL, KT, CHAIN, false, AL, false, 1, false, true>(A);
}

template <int K, int KT>
__global__ __launch_bounds__(128 * ((K + 1) / 2 + 3), 4) void myula_step_pipe_box2_kernel(const StepArgs A) {
  pipe_body<K, 4, KT, false, false, true, false, 2, false, true>(A);
}

template <int PXL, int KT, bool CHAIN, bool AL>
static hipError_t pipe_box_launch_one(const StepArgs& a, hipStream_t st) {
  constexpr int K = 10;
  return pipe_launch<myula_step_pipe_box_kernel<K, PXL, KT, CHAIN, AL>>(pipe_lds_bytes<K, PXL, KT, CHAIN>(), dim3(a.C, pipe_nstrips<K, PXL, KT>(a.W)),
                                                                        dim3(pipe_block(K, 1)), a, st);
}

static hipError_t pipe_box_launch_teams(const StepArgs& a, hipStream_t st) {
  constexpr int K = 10;
  return pipe_launch<myula_step_pipe_box2_kernel<K, 5>>(pipe_teams_lds_bytes<K>(), dim3(a.C), dim3(pipe_block(K, 2)), a, st);
}

template <bool CHAIN, bool AL>
static hipError_t pipe_box_dispatch(const StepArgs& a, int KT, hipStream_t st) {
  return pipe_select(a.W, KT, [&](auto pxl, auto kt) { return pipe_box_launch_one<decltype(pxl)::value, decltype(kt)::value, CHAIN, AL>(a, st); });
}

hipError_t pipe_dispatch_box(const StepArgs& a, int KT, bool chain, int teams, hipStream_t st) {
  if (a.tv.niter != 10 || a.tv_warm || a.tv_aniso || a.rt_kc || !(KT == 0 || KT == 5 || KT == 7) || !(a.box_lo < a.box_hi)) return hipErrorInvalidConfiguration;
  if (teams == 2) return chain ? hipErrorInvalidConfiguration : pipe_box_launch_teams(a, st);
  // AL: the last image column is the last pixel of a lane and rows are 16-byte aligned (as pipe_dispatch_k)
  const bool lastlane = pipe_lastlane(a.W);
  if (chain) return lastlane ? pipe_box_dispatch<true, true>(a, KT, st) : pipe_box_dispatch<true, false>(a, KT, st);
  return lastlane ? pipe_box_dispatch<false, true>(a, KT, st) : pipe_box_dispatch<false, false>(a, KT, st);
}

}  // namespace lmc
