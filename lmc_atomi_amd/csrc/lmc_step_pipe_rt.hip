// RT instantiations of the pipe step kernel (lmc_step_pipe_kernel.h): the TV prox with upstream's per-image early exit (pyproximal.TV's rtol, in force
// at prox_lmc_deconv.py:122 and algs.py:169) as a per-chain number of live pipeline stages, with the primal objectives of the iterates as by-products.
// The K = 10 pipeline serves every iteration cap up to 10 in one launch (stages past a chain's count pass the dual through) and up to 60 as a chain of
// links that hand the dual state over in HBM (the inner prox of the ME-TV term, niter_l2 = 50): a chain leaves in the link that holds its last update,
// the links before it only advance its dual state, the links after it return at once.  The host side that predicts, verifies and re-runs is
// lmc_tv_exit.hip: tv_prox_rt.  A translation unit of its own so that the instantiations compile in parallel with the others.
#include "lmc_step_pipe_kernel.h"

namespace lmc {

bool pipe_rt_supported(const StepArgs& a) {
  if (a.prior_kind != LMC_PRIOR_TV_ISO || a.tv_aniso) return false;     // (the objective of the anisotropic prior is not built)
  const int n = a.tv.niter;
  if (n < 1 || n > 60 || n > kMaxTvIters) return false;
  if (a.tv_in || a.tv_out || a.tv_state_only || a.tv_warm) return false;
  // every width the fixed-count K = 10 kernel covers (the launches here are K = 10 pipelines whatever the cap: ask for that geometry)
  StepArgs g = a;
  g.tv.niter = 10;
  if (!pipe_geometry_ok(g)) return false;
  if (a.f_out || a.g_out) return false;
  // chained links: the pure prox only (every link may be the one some chain leaves in, so none could skip a data term)
  if (n > 10 && (a.data_kind != LMC_DATA_NONE || a.noise_mode != LMC_NOISE_NONE || a.ncvx_kind != LMC_NCVX_NONE || a.extra)) return false;
  return true;
}

// AL as in pipe_dispatch_k (the last image column is a lane's last pixel, rows are 16-byte aligned) -- and one strip: the AL = true kernels sum the
// objectives over whole rows.  Everything else -- unaligned rows, column strips of any alignment -- runs the AL = false kernels, whose objective sums
// carry per-pixel weights (the strip's interior, the last image column).
// The links of a chained prox carry no data term: they are built for KT = 0 only.
template <bool CHAIN, bool AL>
static hipError_t pipe_dispatch_rt_al(const StepArgs& a, int KT, hipStream_t st) {
  return pipe_select(a.W, KT, [&](auto pxl, auto kt) {
    constexpr int PXL = decltype(pxl)::value, KTc = decltype(kt)::value;
    if constexpr (CHAIN && KTc != 0) return hipErrorInvalidConfiguration;
    else return pipe_launch_one<PXL, KTc, CHAIN, 10, false, AL, true>(a, st);
  });
}
template <bool CHAIN>
static hipError_t pipe_dispatch_rt(const StepArgs& a, int KT, hipStream_t st) {
  if (pipe_lastlane(a.W) && a.W <= 512) return pipe_dispatch_rt_al<CHAIN, true>(a, KT, st);
  return pipe_dispatch_rt_al<CHAIN, false>(a, KT, st);
}

hipError_t launch_step_pipe_rt(StepArgs a, hipStream_t st, float* state0, float* state1) {
  if (!pipe_rt_supported(a) || !a.rt_kc || !a.rt_obj || a.rt_stride < a.tv.niter + 1) return hipErrorInvalidConfiguration;
  const int n = a.tv.niter, links = (n + 9) / 10;
  if (links > 1 && (!state0 || !state1)) return hipErrorInvalidConfiguration;
  const int KT = pipe_taps(a);
  a.rt_total = n;
  float* st_buf[2] = {state0, state1};
  for (int j = 0; j < links; ++j) {
    StepArgs b = a;
    b.tv.niter = 10;
    for (int i = 0; i < 10; ++i) b.tv.betas[i] = 10 * j + i < n ? a.tv.betas[10 * j + i] : 0.f;
    b.rt_base = 10 * j;
    if (links > 1) {
      b.tv_in = j > 0 ? st_buf[(j - 1) & 1] : nullptr;
      b.tv_out = j < links - 1 ? st_buf[j & 1] : nullptr;
    }
    const hipError_t e = links > 1 ? pipe_dispatch_rt<true>(b, 0, st) : pipe_dispatch_rt<false>(b, KT, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace lmc
