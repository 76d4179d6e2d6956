// Instantiations of the pipe step kernel (lmc_step_pipe_kernel.h) for the Huber data term (LMC_DATA_HUBER_*, StepArgs::hub; definition: lmc_atomi.h):
//     out = a*x - t*sigma_f H^T clamp(Hx - y, -delta, delta) + b*prox_{gamma TV}(x) + s*xi
// the same pipeline with the L wave clamping the residual row by the threshold row (pipe_body<..., HUB>), with and without the box constraint of the
// prior.  Kernels of their own name, like the box, the anisotropic, the Poisson and the weighted ones:
//   myula_step_pipe_hub_kernel<K = 10, PXL in {4, 8}, KT in {0, 5, 7}, AL>
//   myula_step_pipe_hub_box_kernel<K = 10, PXL in {4, 8}, KT in {0, 5, 7}, AL>
// One team, one launch of exactly 10 dual iterations from the zero dual: no chained form, no two-team form, no early exit, no warm dual, no energy
// by-products, isotropic prior.  Everything else runs in the tile kernel (myula_step_tile_hub_kernel).
#include "lmc_step_pipe_kernel.h"

namespace lmc {

template <int K, int PXL, int KT, bool AL>
__global__ __launch_bounds__(64 * ((K + 1) / 2 + 3), PXL == 8 ? 1 : 2) void myula_step_pipe_hub_kernel(const StepArgs A) {
  pipe_body<K, PXL, KT, false, false, AL, false, 1, false, false, false, false, false, true>(A);
}

template <int K, int PXL, int KT, bool AL>
__global__ __launch_bounds__(64 * ((K + 1) / 2 + 3), PXL == 8 ? 1 : 2) void myula_step_pipe_hub_box_kernel(const StepArgs A) {
  pipe_body<K, PXL, KT, false, false, AL, false, 1, false, true, false, false, false, true>(A);
}

template <bool BOX, bool AL>
static hipError_t pipe_hub_dispatch(const StepArgs& a, int KT, hipStream_t st) {
  constexpr int K = 10;
  return pipe_select(a.W, KT, [&](auto pxl, auto kt) {
    constexpr int PXL = decltype(pxl)::value, KTc = decltype(kt)::value;
    const dim3 grid(a.C, pipe_nstrips<K, PXL, KTc>(a.W)), block(pipe_block(K, 1));
    if constexpr (BOX) return pipe_launch<myula_step_pipe_hub_box_kernel<K, PXL, KTc, AL>>(pipe_lds_bytes<K, PXL, KTc, false>(), grid, block, a, st);
    else return pipe_launch<myula_step_pipe_hub_kernel<K, PXL, KTc, AL>>(pipe_lds_bytes<K, PXL, KTc, false>(), grid, block, a, st);
  });
}

hipError_t pipe_dispatch_hub(const StepArgs& a, int KT, hipStream_t st) {
  if (!a.hub || a.pois || a.wl2 || a.tv.niter != 10 || a.tv_warm || a.tv_aniso || a.rt_kc || a.tv_in || a.tv_out || a.f_out || a.g_out ||
      !(KT == 0 || KT == 5 || KT == 7) || a.data_kind == LMC_DATA_MASK || (a.box && !(a.box_lo < a.box_hi)))
    return hipErrorInvalidConfiguration;
  // AL: the last image column is the last pixel of a lane and rows are 16-byte aligned (as pipe_dispatch_k)
  const bool lastlane = pipe_lastlane(a.W);
  if (a.box) return lastlane ? pipe_hub_dispatch<true, true>(a, KT, st) : pipe_hub_dispatch<true, false>(a, KT, st);
  return lastlane ? pipe_hub_dispatch<false, true>(a, KT, st) : pipe_hub_dispatch<false, false>(a, KT, st);
}

}  // namespace lmc
