// Instantiations of the pipe step kernel (lmc_step_pipe_kernel.h) for the data terms that read a second plane of y (DataTerm, StepArgs::term; definitions:
// lmc_atomi.h):
//     out = a*x - t*sigma_f H^T psi(Hx) + b*prox_{gamma TV}(x) + s*xi
//   Poisson (LMC_DATA_POISSON_*)   psi = rho = phi' of the extended Kullback-Leibler term, second plane: the background beta
//   weighted (LMC_DATA_WL2_*)      psi = w (Hx - y), second plane: the weights w
//   Huber (LMC_DATA_HUBER_*)       psi = clamp(Hx - y, -delta, delta), second plane: the thresholds delta
// the same pipeline with the L wave forming psi where it forms Hx - y (pipe_body<..., TERM>), with and without the box constraint of the prior
// (for Poisson positivity, bounds = (0, inf), is what the model is meant to run with).  Kernels of their own name, like the box and the anisotropic ones:
//   myula_step_pipe_{pois,wl2,hub}_kernel<K = 10, PXL in {4, 8}, KT in {0, 5, 7}, AL>
//   myula_step_pipe_{pois,wl2,hub}_box_kernel<K = 10, PXL in {4, 8}, KT in {0, 5, 7}, AL>
// One team, one launch of exactly 10 dual iterations from the zero dual: no chained form, no two-team form, no early exit, no warm dual, no energy
// by-products, isotropic prior.  Everything else runs in the tile kernel (myula_step_tile_{pois,wl2,hub}_kernel).
#include "lmc_step_pipe_kernel.h"

namespace lmc {

#define LMC_PIPE_TERM_BOUNDS __launch_bounds__(64 * ((K + 1) / 2 + 3), PXL == 8 ? 1 : 2)
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_pois_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, false, kTermPois>(A); }
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_pois_box_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, true, kTermPois>(A); }
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_wl2_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, false, kTermWl2>(A); }
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_wl2_box_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, true, kTermWl2>(A); }
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_hub_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, false, kTermHub>(A); }
template <int K, int PXL, int KT, bool AL>
__global__ LMC_PIPE_TERM_BOUNDS void myula_step_pipe_hub_box_kernel(const StepArgs A) { pipe_body<K, PXL, KT, false, false, AL, false, 1, false, true, kTermHub>(A); }
#undef LMC_PIPE_TERM_BOUNDS

template <int TERM, bool BOX, int K, int PXL, int KT, bool AL>
static constexpr auto pipe_term_kernel() {
  if constexpr (TERM == kTermPois) return BOX ? myula_step_pipe_pois_box_kernel<K, PXL, KT, AL> : myula_step_pipe_pois_kernel<K, PXL, KT, AL>;
  else if constexpr (TERM == kTermWl2) return BOX ? myula_step_pipe_wl2_box_kernel<K, PXL, KT, AL> : myula_step_pipe_wl2_kernel<K, PXL, KT, AL>;
  else if constexpr (TERM == kTermHub) return BOX ? myula_step_pipe_hub_box_kernel<K, PXL, KT, AL> : myula_step_pipe_hub_kernel<K, PXL, KT, AL>;
}

template <int TERM, bool BOX, bool AL>
static hipError_t pipe_term_launch(const StepArgs& a, int KT, hipStream_t st) {
  constexpr int K = 10;
  return pipe_select(a.W, KT, [&](auto pxl, auto kt) {
    constexpr int PXL = decltype(pxl)::value, KTc = decltype(kt)::value;
    const dim3 grid(a.C, pipe_nstrips<K, PXL, KTc>(a.W)), block(pipe_block(K, 1));
    return pipe_launch<pipe_term_kernel<TERM, BOX, K, PXL, KTc, AL>()>(pipe_lds_bytes<K, PXL, KTc, false>(), grid, block, a, st);
  });
}

template <int TERM>
static hipError_t pipe_term_forms(const StepArgs& a, int KT, hipStream_t st) {
  // AL: the last image column is the last pixel of a lane and rows are 16-byte aligned (as pipe_dispatch_k)
  const bool lastlane = pipe_lastlane(a.W);
  if (a.box) return lastlane ? pipe_term_launch<TERM, true, true>(a, KT, st) : pipe_term_launch<TERM, true, false>(a, KT, st);
  return lastlane ? pipe_term_launch<TERM, false, true>(a, KT, st) : pipe_term_launch<TERM, false, false>(a, KT, st);
}

hipError_t pipe_dispatch_term(const StepArgs& a, int KT, hipStream_t st) {
  if (a.term == kTermL2 || a.tv.niter != 10 || a.tv_warm || a.tv_aniso || a.rt_kc || a.tv_in || a.tv_out || a.f_out || a.g_out || !(KT == 0 || KT == 5 || KT == 7) ||
      (a.term != kTermPois && a.data_kind == LMC_DATA_MASK) || (a.box && !(a.box_lo < a.box_hi)))     // only the Poisson term has a mask operator
    return hipErrorInvalidConfiguration;
  switch (a.term) {
    case kTermPois: return pipe_term_forms<kTermPois>(a, KT, st);
    case kTermWl2: return pipe_term_forms<kTermWl2>(a, KT, st);
    case kTermHub: return pipe_term_forms<kTermHub>(a, KT, st);
    default: return hipErrorInvalidConfiguration;
  }
}

}  // namespace lmc
