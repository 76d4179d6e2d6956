// The TV proxes with upstream's per-image early exit (decided on the device, or pass by pass), the inner prox of the ME-TV term and its
// envelope.
#include <cstring>

#include "lmc_host.h"

namespace lmc::host {

bool needs_tv_state(const Problem& q) {
  return ((q.prior_kind == LMC_PRIOR_TV_ISO || q.prior_kind == LMC_PRIOR_TV_ANISO) && (q.tv_niter > 12 || (q.tv_rtol > 0.f && q.tv_niter > 10))) ||
         (q.ncvx_kind == LMC_NCVX_ME_TV && (q.ncvx_aniso || q.ncvx_niter > 12 || (q.ncvx_rtol > 0.f && q.ncvx_niter > 10)));
}

// The TV prox inside A (a complete StepArgs: prox only, or the whole fused update when A.tv.niter <= 10) with upstream's per-image early exit,
// decided on the device: every chain runs with the pass count it left in last time (rt.pred), the launch leaves the primal objectives of
// the iterates behind, tv_rt_decide replays upstream's test on them, and the chains whose prediction was wrong run again -- with the exact
// count when the objectives already show it, else with one pass more, then with all passes (whose objectives show it) and then once more.
// Four rounds settle every chain; the workgroups of settled chains return at once, so the later rounds cost a few microseconds when the
// predictions hold, and a chained prox re-runs from the link the change lies in, not from its first.  No host synchronisation.
// (lmc_ops.hip: tv_rt_begin / tv_rt_decide; lmc_step_pipe_rt.hip.)
constexpr int kRtRounds = 4;
int tv_prox_rt(lmc::StepArgs A, RtState& rt, float rtol, float* st0, float* st1, hipStream_t st) {
  const int niter = A.tv.niter;
  if (!rt.kc || rt.n < (size_t)A.C || rt.stride < niter + 1) return fail(LMC_E_STATE, "early-exit buffers are missing");
  A.rt_kc = rt.kc; A.rt_start = rt.start; A.rt_obj = rt.obj; A.rt_stride = rt.stride;
  HIP_TRY(lmc::launch_tv_rt_begin(A.C, rt.pred, rt.kc, rt.start, rt.obj, rt.stride, niter, st));
  for (int round = 0; round < kRtRounds; ++round) {
    hipError_t e = lmc::launch_step_pipe_rt(A, st, st0, st1);
    if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "the device-side early exit of the TV prox does not cover this configuration");
    HIP_TRY(e);
    HIP_TRY(lmc::launch_tv_rt_decide(A.C, rt.kc, rt.start, rt.pred, rt.obj, rt.stride, niter, (double)rtol, round, rt.reruns + round, st));
  }
  return LMC_OK;
}

// out <- prox_{gam TV_1D}(x) of the n flattened images (N = H W entries each) by `niter` 1-D FGP iterations (lmc_ops.hip: tv1d_*), with upstream's early
// exit when rtol > 0 (pass by pass: the host reads the number of images still iterating after every pass).  buf: 4 n N floats (dual, dual, projected dual,
// iterate); obj: 2 n doubles; flag: n + 1 ints.
int tv1d_prox(const float* x, float* out, int64_t n, size_t N, float gam, int niter, float rtol, float* buf, double* obj, int* flag, hipStream_t st) {
  const size_t tot = (size_t)n * N;
  float *rr[2] = {buf, buf + tot}, *p = buf + 2 * tot, *tmp = buf + 3 * tot;
  float betas[lmc::kMaxTvIters];
  default_betas(betas, niter);
  const float cstep = 0.25f / gam;
  double *prev = obj, *cur = obj + n;
  int* n_active = flag + n;
  HIP_TRY(hipMemsetAsync(buf, 0, sizeof(float) * 3 * tot, st));
  HIP_TRY(hipMemsetAsync(obj, 0, sizeof(double) * 2 * n, st));
  HIP_TRY(hipMemsetAsync(flag, 0xFF, sizeof(int) * n, st));
  for (int j = 0; j <= niter; ++j) {
    const float* r_now = rr[j & 1];
    if (rtol > 0.f || j == niter) HIP_TRY(lmc::launch_tv1d_sol(x, r_now, tmp, n, N, gam, flag, st));
    if (j == niter) {                                                        // out of passes: the rest take sol_niter untested
      HIP_TRY(lmc::launch_tv_rtol_select(tmp, out, flag, -1, n, N, st));
      break;
    }
    if (rtol > 0.f) {
      HIP_TRY(lmc::launch_tv1d_objective(x, tmp, n, N, gam, flag, cur, st));
      HIP_TRY(hipMemsetAsync(n_active, 0, sizeof(int), st));
      HIP_TRY(lmc::launch_tv_rtol_decide(n, prev, cur, flag, j, (double)rtol, n_active, st));
      if (j > 0) HIP_TRY(lmc::launch_tv_rtol_select(tmp, out, flag, j, n, N, st));
      int active = 0;
      HIP_TRY(hipMemcpyAsync(&active, n_active, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (active == 0) break;
    }
    HIP_TRY(lmc::launch_tv1d_iter(x, r_now, p, rr[(j & 1) ^ 1], n, N, gam, cstep, betas[j], flag, st));
  }
  return LMC_OK;
}

// extra <- prox_{gamma TV}(x) with ncvx_niter dual iterations (the inner prox of the ME-TV term, algs.py:169,282)
int me_tv_prox(const Problem& q, const float* x, float* extra, int64_t n_img, float* state0, float* state1, hipStream_t st, RtState* rt) {
  lmc::StepArgs A;
  std::memset(&A, 0, sizeof A);
  A.H = q.H; A.W = q.W; A.C = (int)n_img;
  A.data_kind = LMC_DATA_NONE;
  A.prior_kind = LMC_PRIOR_TV_ISO;
  A.tv.niter = q.ncvx_niter;
  A.tv.gamma = q.ncvx_gamma;          // g_gamma = TV(dims, sigma = 1) evaluated at prox parameter gamma (algs.py:169,282)
  A.tv.c = 0.125f / q.ncvx_gamma;
  default_betas(A.tv.betas, q.ncvx_niter);
  A.a = 0.f; A.t = 0.f; A.b = 1.f; A.s = 0.f;
  A.noise_mode = LMC_NOISE_NONE;
  A.x_in = x; A.x_out = extra;
  A.y = x; A.mask = x; A.noise = x;
  if (q.ncvx_niter == 0) {     // lagged output of a 1-iteration prox: x itself
    HIP_TRY(hipMemcpyAsync(extra, x, sizeof(float) * (size_t)n_img * q.H * q.W, hipMemcpyDeviceToDevice, st));
    return LMC_OK;
  }
  if (q.ncvx_aniso) {          // algs.py:170: the 1-D TV of the flattened image
    if (!state0) return fail(LMC_E_STATE, "anisotropic ME-TV: work buffers are missing");
    Scratch& sc = scratch_here();
    HIP_TRY(sc.need_dbl(3 * (size_t)n_img + 2));
    return tv1d_prox(x, extra, n_img, (size_t)q.H * q.W, q.ncvx_gamma, q.ncvx_niter, q.ncvx_rtol, state0, sc.dbl, reinterpret_cast<int*>(sc.dbl + 2 * n_img), st);
  }
  if (q.ncvx_rtol > 0.f) {     // the class's own rtol (algs.py:130,169): per-chain early exit
    if (rt && q.tv_exit_path == 0 && lmc::pipe_rt_supported(A)) return tv_prox_rt(A, *rt, q.ncvx_rtol, state0, state1, st);     // on the device
    // elsewhere (images up to 128 columns wide, more than 60 passes, tv_exit_path = 1): pass by pass, as the TV prior's prox (synchronises the stream)
    Problem qt;
    qt.H = q.H; qt.W = q.W;
    qt.prior_kind = LMC_PRIOR_TV_ISO; qt.prior_sigma = 1.f; qt.tv_niter = q.ncvx_niter; qt.tv_step = 0.125f; qt.tv_rtol = q.ncvx_rtol;
    default_betas(qt.betas, q.ncvx_niter);
    qt.variant = q.variant;
    Scratch& sc = scratch_here();
    HIP_TRY(sc.need_rtmp((size_t)n_img * q.H * q.W));
    HIP_TRY(sc.need_dbl(3 * (size_t)n_img + 2));
    return tv_prox_rtol(qt, q.ncvx_gamma, x, extra, sc.rtmp, sc.dbl, reinterpret_cast<int*>(sc.dbl + 2 * n_img), n_img, state0, state1, st);
  }
  hipError_t e = launch_step(A, variant_of(q), st, nullptr, state0, state1);
  if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "no kernel covers the inner TV prox of the ME-TV term");
  HIP_TRY(e);
  return LMC_OK;
}


// prox_{pt g}(x), g = sigma TV, with upstream's per-image early exit (lmc_problem.tv_rtol > 0; pyproximal.TV.prox as restated by the
// CPU checker's tv_prox_fgp): at the top of pass j the iterate sol_j = x - gam div(r_j) (j dual updates) and its primal objective
// are formed; an image leaves with sol_j as soon as the relative change of the objective drops below rtol (never in pass 0); after
// tv_niter updates the iterate is returned untested.  Exact, pass by pass, for the whole batch: pass j's iterate is ONE fused launch
// with j dual iterations from the zero dual (the stages of a longer launch compute the same values), the objective a second one; images
// that have left keep their iterate (flag / select).  The host reads the number of images still iterating after every pass -- this
// path synchronises the stream, the fixed-count path (tv_rtol = 0) never does.  Typical MYULA iterates leave after 2-4 passes.
// sol, tmp: [n][H][W]; obj: 2n doubles (previous, current); flag: n + 1 ints (pass an image left in, -1 = iterating; then the counter).
int tv_prox_rtol(const Problem& q, float pt, const float* x, float* sol, float* tmp, double* obj, int* flag, int64_t n, float* st0, float* st1,
                 hipStream_t st) {
  const float gam = pt * q.prior_sigma;
  if (!(gam > 0.f)) return fail(LMC_E_INVALID, "TV prox parameter must be > 0 (got %g)", (double)gam);
  const size_t img = (size_t)q.H * q.W;
  double *prev = obj, *cur = obj + n;
  int* n_active = flag + n;
  HIP_TRY(hipMemsetAsync(obj, 0, sizeof(double) * 2 * n, st));
  HIP_TRY(hipMemsetAsync(flag, 0xFF, sizeof(int) * n, st));                  // -1: every image iterating
  const int K = q.tv_niter;
  for (int j = 0; j <= K; ++j) {
    const float* it = x;                                                     // pass 0: sol_0 = x
    if (j > 0) {
      Problem qj = q;
      qj.tv_niter = j;
      qj.ncvx_kind = LMC_NCVX_NONE;
      lmc::StepArgs A;
      int rc = make_step_args(qj, 0.f, 0.f, 1.f, pt, 0.f, A);
      if (rc) return rc;
      A.C = (int)n; A.x_in = x; A.x_out = tmp;
      sanitize_pointers(A);
      hipError_t e = launch_step(A, 0 /* auto: the passes have 1, 2, 3 ... dual iterations, no single variant covers them all */, st, nullptr, st0, st1);
      if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "no step-kernel variant covers a TV prox with %d dual iterations", j);
      HIP_TRY(e);
      it = tmp;
    }
    if (j == K) {                                                            // out of passes: the rest take sol_K untested
      HIP_TRY(lmc::launch_tv_rtol_select(it, sol, flag, -1, n, img, st));
      break;
    }
    HIP_TRY(lmc::launch_tv_objective(x, it, n, q.H, q.W, gam, flag, cur, st));
    HIP_TRY(hipMemsetAsync(n_active, 0, sizeof(int), st));
    HIP_TRY(lmc::launch_tv_rtol_decide(n, prev, cur, flag, j, (double)q.tv_rtol, n_active, st));
    if (j > 0) HIP_TRY(lmc::launch_tv_rtol_select(it, sol, flag, j, n, img, st));
    int active = 0;
    HIP_TRY(hipMemcpyAsync(&active, n_active, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (active == 0) break;
  }
  return LMC_OK;
}

// The TV PRIOR's prox with the early exit on the device.  A: the complete fused update (x_in, x_out, data term, noise ...).  Returns 1 when the
// update has been computed (up to 10 passes: the exit lives inside the fused step launch), 0 when the prox alone went to `proxbuf` and A now
// consumes it as a ready-made prox (more than 10 passes, or a data term the pipeline does not cover: the caller launches the step), 2 when the
// device path does not cover the problem (the caller takes the pass-by-pass path), or a negative status.
int tv_prior_rt(const Problem& q, float pt, lmc::StepArgs& A, RtState& rt, float* proxbuf, float* st0, float* st1, hipStream_t st) {
  if (A.tv.niter <= 10 && lmc::pipe_rt_supported(A)) {
    const int rc = tv_prox_rt(A, rt, q.tv_rtol, st0, st1, st);
    return rc ? rc : 1;
  }
  Problem qp = q;
  qp.ncvx_kind = LMC_NCVX_NONE;
  lmc::StepArgs P;
  int rc = make_step_args(qp, 0.f, 0.f, 1.f, pt, 0.f, P);
  if (rc) return rc;
  P.C = A.C; P.x_in = A.x_in; P.x_out = proxbuf;
  sanitize_pointers(P);
  if (!proxbuf || !lmc::pipe_rt_supported(P)) return 2;
  rc = tv_prox_rt(P, rt, q.tv_rtol, st0, st1, st);
  if (rc) return rc;
  A.prior_kind = LMC_PRIOR_NONE;
  A.prox_ext = proxbuf;
  return 0;
}
// which of the two the sampler / call will take: 1 fused, 0 prox alone, 2 not covered
int tv_prior_rt_mode(const Problem& q, const lmc::StepArgs& A_probe, float pt) {
  if (q.tv_exit_path != 0) return 2;
  if (A_probe.tv.niter <= 10 && lmc::pipe_rt_supported(A_probe)) return 1;
  Problem qp = q;
  qp.ncvx_kind = LMC_NCVX_NONE;
  lmc::StepArgs P;
  if (make_step_args(qp, 0.f, 0.f, 1.f, pt, 0.f, P)) return 2;
  P.C = A_probe.C;
  return lmc::pipe_rt_supported(P) ? 0 : 2;
}

lmc::EnergyArgs energy_args(const Problem& q) {
  lmc::EnergyArgs E;
  // (a Poisson or a weighted Gaussian data term: none here -- f stays 0 and pois_energy / wl2_energy adds its value)
  E.H = q.H; E.W = q.W; E.data_kind = (q.pois || q.wl2 || q.psf.on || q.fft.on) ? LMC_DATA_NONE : q.data_kind; E.sigma_f = q.sigma_f; E.y = q.y; E.mask = q.mask;
  E.blur = q.taps; E.prior_kind = q.prior_kind; E.prior_sigma = q.prior_sigma;
  E.ncvx_kind = q.ncvx_kind == LMC_NCVX_MC_TV ? LMC_NCVX_MC_TV : LMC_NCVX_NONE;   // ME-TV envelope: me_tv_energy
  E.ncvx_lambda = q.ncvx_lambda; E.ncvx_gamma = q.ncvx_gamma;
  return E;
}

// after launch_energies(..., energy_args(q), f_out, ...): f_out += the Poisson data term's value (nothing for the Gaussian terms)
int pois_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st) {
  if (!q.pois || q.psf.on || !f_out) return LMC_OK;
  lmc::EnergyArgs E = energy_args(q);
  E.data_kind = q.data_kind;
  E.ncvx_kind = LMC_NCVX_NONE;
  HIP_TRY(lmc::launch_energy_pois(x, n_img, E, f_out, st));
  return LMC_OK;
}

// the same for the weighted Gaussian data term (LMC_DATA_WL2_*)
int wl2_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st) {
  if (!q.wl2 || q.psf.on || !f_out) return LMC_OK;
  lmc::EnergyArgs E = energy_args(q);
  E.data_kind = q.data_kind;
  E.ncvx_kind = LMC_NCVX_NONE;
  HIP_TRY(lmc::launch_energy_wl2(x, n_img, E, f_out, st));
  return LMC_OK;
}

// g_out = the value of the wavelet prior (LMC_PRIOR_WAVELET_L1; launch_energies leaves 0 there), from the workspace q.wav carries
int wavelet_energy(const Problem& q, const float* x, int64_t n_img, double* g_out, hipStream_t st) {
  if (!q.wav.on || !g_out) return LMC_OK;
  HIP_TRY(lmc::launch_wavelet_value(x, n_img, q.H, q.W, q.wav.p, q.wav.levels, q.prior_sigma, q.wav.ws, q.wav.part, g_out, st));
  return LMC_OK;
}

// the same for a large PSF (LMC_DATA_PSF with its pois / wl2 flags): deterministic partial sums, from the scratch of the current device
int psf_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st) {
  if (!q.psf.on || !f_out) return LMC_OK;
  Scratch& sc = scratch_here();
  HIP_TRY(sc.need_dbl(lmc::psf_energy_partials(n_img, q.H, q.W)));
  HIP_TRY(lmc::launch_psf_energy(q.psf, q.pois ? 2 : q.wl2 ? 1 : 0, x, q.y, n_img, q.H, q.W, q.sigma_f, sc.dbl, f_out, st));
  return LMC_OK;
}

// the same for the spectral data term (LMC_DATA_SPECTRAL): row transform, column transform and residuals, the fixed-order sum
int spectral_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st) {
  if (!q.fft.on || !f_out) return LMC_OK;
  HIP_TRY(lmc::launch_fft_value(q.fft, x, n_img, q.H, q.W, q.sigma_f, f_out, st));
  return LMC_OK;
}

// f_out -= lambda * ( TV(prox) + ||x - prox||^2 / (2 gamma) ),  prox = prox_{gamma TV}(x)    (algs.py:178-190, ME-TV)
int me_tv_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, float* extra, float* st0, float* st1,
                 double* dbl /* 2*n_img */, hipStream_t st, RtState* rt) {
  int rc = me_tv_prox(q, x, extra, n_img, st0, st1, st, rt);
  if (rc) return rc;
  lmc::EnergyArgs E;
  std::memset(&E, 0, sizeof E);
  E.H = q.H; E.W = q.W; E.data_kind = LMC_DATA_NONE; E.prior_kind = LMC_PRIOR_TV_ISO; E.prior_sigma = 1.f;
  if (q.ncvx_aniso) {                                                                    // TV_1D(prox) of the flattened image
    HIP_TRY(hipMemsetAsync(dbl, 0, sizeof(double) * n_img, st));
    HIP_TRY(lmc::launch_tv1d_objective(extra, extra, n_img, (size_t)q.H * q.W, 1.f, nullptr, dbl, st));
  } else
  HIP_TRY(lmc::launch_energies(extra, n_img, E, nullptr, dbl, st));                       // TV(prox)
  HIP_TRY(lmc::launch_sqdiff(x, extra, n_img, (size_t)q.H * q.W, dbl + n_img, st));      // ||x - prox||^2
  HIP_TRY(lmc::launch_axpy_env(f_out, dbl, dbl + n_img, n_img, q.ncvx_lambda, q.ncvx_gamma, st));
  return LMC_OK;
}

}  // namespace lmc::host
