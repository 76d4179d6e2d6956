// The TV proxes with upstream's per-image early exit (decided on the device, or pass by pass), the inner prox of the ME-TV term and its
// envelope, and the energies of a problem.  Every function here works in the buffers of the Workspace it is given, as prepare() sized them.
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
static int tv_prox_rt(lmc::StepArgs A, RtState& rt, float rtol, Workspace& ws, hipStream_t st) {
  const int niter = A.tv.niter;
  if (!rt.kc || rt.n < (size_t)A.C || rt.stride < niter + 1) return fail(LMC_E_STATE, "early-exit buffers are missing");
  A.rt_kc = rt.kc; A.rt_start = rt.start; A.rt_obj = rt.obj; A.rt_stride = rt.stride;
  HIP_TRY(lmc::launch_tv_rt_begin(A.C, rt.pred, rt.kc, rt.start, rt.obj, rt.stride, niter, st));
  for (int round = 0; round < kRtRounds; ++round) {
    hipError_t e = lmc::launch_step_pipe_rt(A, st, ws.state[0].p, ws.state[1].p);
    if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "the device-side early exit of the TV prox does not cover this configuration");
    HIP_TRY(e);
    HIP_TRY(lmc::launch_tv_rt_decide(A.C, rt.kc, rt.start, rt.pred, rt.obj, rt.stride, niter, (double)rtol, round, rt.reruns + round, st));
  }
  return LMC_OK;
}

// out <- prox_{gam TV_1D}(x) of the n flattened images (N = H W entries each) by `niter` 1-D FGP iterations (lmc_ops.hip: tv1d_*), with upstream's early
// exit when rtol > 0 (pass by pass: the host reads the number of images still iterating after every pass).  In ws: the first dual state as 4 n N floats
// (dual, dual, projected dual, iterate) and the exit scalars.
static int tv1d_prox(const float* x, float* out, int64_t n, size_t N, float gam, int niter, float rtol, Workspace& ws, hipStream_t st) {
  const size_t tot = (size_t)n * N;
  float* buf = ws.state[0].p;
  double* obj = ws.exit_obj();
  int* flag = ws.exit_flag(n);
  if (!buf || !obj) return fail(LMC_E_STATE, "anisotropic ME-TV: work buffers are missing");
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

// the launch of prox_{gamma TV} with ncvx_niter dual iterations on n_img images (the inner prox of the ME-TV term, algs.py:169,282), without its pointers
static lmc::StepArgs me_tv_args(const Problem& q, int64_t n_img) {
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
  return A;
}

bool me_tv_exit_on_device(const Problem& q, int64_t n_img) { return q.tv_exit_path == 0 && lmc::pipe_rt_supported(me_tv_args(q, n_img)); }

int me_tv_prox(const Problem& q, const float* x, int64_t n_img, Workspace& ws, hipStream_t st) {
  float* extra = ws.extra.p;
  if (q.ncvx_niter == 0) {     // lagged output of a 1-iteration prox: x itself
    HIP_TRY(hipMemcpyAsync(extra, x, sizeof(float) * (size_t)n_img * q.H * q.W, hipMemcpyDeviceToDevice, st));
    return LMC_OK;
  }
  if (q.ncvx_aniso)            // algs.py:170: the 1-D TV of the flattened image
    return tv1d_prox(x, extra, n_img, (size_t)q.H * q.W, q.ncvx_gamma, q.ncvx_niter, q.ncvx_rtol, ws, st);
  lmc::StepArgs A = me_tv_args(q, n_img);
  A.x_in = x; A.x_out = extra;
  A.y = x; A.mask = x; A.noise = x;
  if (q.ncvx_rtol > 0.f) {     // the class's own rtol (algs.py:130,169): per-chain early exit
    if (me_tv_exit_on_device(q, n_img)) return tv_prox_rt(A, ws.rt_me, q.ncvx_rtol, ws, st);
    // elsewhere (images up to 128 columns wide, more than 60 passes, tv_exit_path = 1): pass by pass, as the TV prior's prox (synchronises the stream)
    Problem qt;
    qt.H = q.H; qt.W = q.W;
    qt.prior_kind = LMC_PRIOR_TV_ISO; qt.prior_sigma = 1.f; qt.tv_niter = q.ncvx_niter; qt.tv_step = 0.125f; qt.tv_rtol = q.ncvx_rtol;
    default_betas(qt.betas, q.ncvx_niter);
    qt.variant = q.variant;
    return tv_prox_rtol(qt, q.ncvx_gamma, x, extra, n_img, ws, st);
  }
  hipError_t e = launch_step(A, q, ws, st, nullptr);
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
// sol: [n][H][W].  In ws: rtmp, the iterate of a pass, [n][H][W]; the exit scalars -- 2n objectives (previous, current), then n + 1 ints (the pass an
// image left in, -1 = iterating; then the counter).
int tv_prox_rtol(const Problem& q, float pt, const float* x, float* sol, int64_t n, Workspace& ws, hipStream_t st) {
  const float gam = pt * q.prior_sigma;
  if (!(gam > 0.f)) return fail(LMC_E_INVALID, "TV prox parameter must be > 0 (got %g)", (double)gam);
  const size_t img = (size_t)q.H * q.W;
  float* tmp = ws.rtmp.p;
  double* obj = ws.exit_obj();
  int* flag = ws.exit_flag(n);
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
      hipError_t e = launch_step(A, 0 /* auto: the passes have 1, 2, 3 ... dual iterations, no single variant covers them all */, q, ws, st, nullptr);
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
// update has been computed (up to 10 passes: the exit lives inside the fused step launch), 0 when the prox alone went to ws.prox and A now
// consumes it as a ready-made prox (more than 10 passes, or a data term the pipeline does not cover: the caller launches the step), 2 when the
// device path does not cover the problem (the caller takes the pass-by-pass path), or a negative status.
int tv_prior_rt(const Problem& q, float pt, lmc::StepArgs& A, Workspace& ws, hipStream_t st) {
  float* proxbuf = ws.prox.p;
  if (A.tv.niter <= 10 && lmc::pipe_rt_supported(A)) {
    const int rc = tv_prox_rt(A, ws.rt_tv, q.tv_rtol, ws, st);
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
  rc = tv_prox_rt(P, ws.rt_tv, q.tv_rtol, ws, st);
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

static lmc::EnergyArgs energy_args(const Problem& q) {
  lmc::EnergyArgs E;
  // (a data term with an energy launch of its own -- Poisson, weighted Gaussian, Huber, large PSF, spectral, Radon, SENSE: none here, f stays 0 and problem_energies adds its value)
  E.H = q.H; E.W = q.W; E.data_kind = (q.term != lmc::kTermL2 || q.psf.on || q.fft.on || q.radon.on || q.sense.on) ? LMC_DATA_NONE : q.data_kind; E.sigma_f = q.sigma_f; E.y = q.y; E.mask = q.mask;
  E.blur = q.taps; E.prior_kind = q.prior_kind; E.prior_sigma = q.prior_sigma;
  E.ncvx_kind = q.ncvx_kind == LMC_NCVX_MC_TV ? LMC_NCVX_MC_TV : LMC_NCVX_NONE;   // ME-TV envelope: me_tv_energy
  E.ncvx_lambda = q.ncvx_lambda; E.ncvx_gamma = q.ncvx_gamma;
  return E;
}

// f_out -= lambda * ( TV(prox) + ||x - prox||^2 / (2 gamma) ),  prox = prox_{gamma TV}(x)    (algs.py:178-190, ME-TV); the two sums in ws.dbl
static int me_tv_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, Workspace& ws, hipStream_t st) {
  int rc = me_tv_prox(q, x, n_img, ws, st);
  if (rc) return rc;
  const float* extra = ws.extra.p;
  double* dbl = ws.dbl.p;
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

// The general energy launch (every prior but the transforms; the Gaussian data terms of the blur / pointwise operators; the MC-TV term), then what has a
// launch of its own: f of the Poisson, weighted and Huber terms, of a large PSF (deterministic partial sums in ws.dbl) and of the spectral term (row transform,
// column transform and residuals, a fixed-order sum; q.fft carries the buffers); g of the Haar and wavelet priors (launch_energies leaves 0 there; q.wav
// carries the workspace); the ME-TV envelope off f.
int problem_energies(const Problem& q, const float* x, int64_t n_img, double* f_out, double* g_out, Workspace& ws, hipStream_t st) {
  HIP_TRY(lmc::launch_energies(x, n_img, energy_args(q), f_out, g_out, st));
  if (f_out && q.term != lmc::kTermL2 && !q.psf.on && !q.radon.on) {
    lmc::EnergyArgs E = energy_args(q);
    E.data_kind = q.data_kind;
    E.ncvx_kind = LMC_NCVX_NONE;
    HIP_TRY(lmc::launch_energy_term(q.term, x, n_img, E, f_out, st));
  }
  if (f_out && q.psf.on) HIP_TRY(lmc::launch_psf_energy(q.psf, q.term, x, q.y, n_img, q.H, q.W, q.sigma_f, ws.dbl.p, f_out, st));
  if (f_out && q.fft.on) HIP_TRY(lmc::launch_fft_value(q.fft, x, n_img, q.H, q.W, q.sigma_f, f_out, st));
  if (f_out && q.sense.on) HIP_TRY(lmc::launch_sense_value(q.sense, x, n_img, q.H, q.W, q.sigma_f, f_out, st));      // (coil by coil, added in coil order)
  if (f_out && q.radon.on) HIP_TRY(lmc::launch_radon_energy(q.radon, q.term, x, q.y, n_img, q.H, q.W, q.sigma_f, ws.dbl.p, f_out, st));
  if (g_out && q.prior_kind == LMC_PRIOR_HAAR_L1) HIP_TRY(lmc::launch_haar_value(x, n_img, q.H, q.W, q.prior_sigma, g_out, st));
  if (g_out && q.wav.on) HIP_TRY(lmc::launch_wavelet_value(x, n_img, q.H, q.W, q.wav.p, q.wav.levels, q.prior_sigma, q.wav.ws, q.wav.part, g_out, st));
  if (f_out && q.ncvx_kind == LMC_NCVX_ME_TV) return me_tv_energy(q, x, n_img, f_out, ws, st);
  return LMC_OK;
}

}  // namespace lmc::host
