// lmc_problem -> Problem (the argument checks of every entry point that takes a problem), the StepArgs of one update, prepare() (the work buffers
// a problem needs and the binding of its operators to them), the library defaults and the step-kernel dispatch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lmc_host.h"

namespace lmc {
int pipe_taps(StepArgs& a);      // lmc_step_pipe.hip: centred taps of the pipe kernels, returns KT
}

namespace lmc::host {

int fill_taps(lmc::BlurTaps& T, const float* h, int kh, int kw, int oy, int ox) {
  if (!h) return fail(LMC_E_INVALID, "blur kernel pointer is NULL");
  if (kh < 1 || kw < 1 || kh > lmc::kMaxBlur || kw > lmc::kMaxBlur)
    return fail(LMC_E_UNSUPPORTED, "blur kernel %dx%d outside 1..%d", kh, kw, lmc::kMaxBlur);
  if (oy < 0 || oy >= kh || ox < 0 || ox >= kw) return fail(LMC_E_INVALID, "blur offset (%d,%d) outside kernel", oy, ox);
  T.kh = kh; T.kw = kw; T.oy = oy; T.ox = ox;
  std::memset(T.h, 0, sizeof T.h);
  std::memcpy(T.h, h, sizeof(float) * kh * kw);
  return LMC_OK;
}

// default momentum table: t_k = (1 + sqrt(4 t_{k-1}^2))/2 (pyproximal.TV / UNLocBoX), beta_k = (t_{k-1}-1)/t_k
void default_betas(float* b, int n) {
  double t = 1.0;
  for (int k = 0; k < n; ++k) {
    const double tn = (1.0 + std::sqrt(4.0 * t * t)) / 2.0;
    b[k] = (float)((t - 1.0) / tn);
    t = tn;
  }
}

// The step of the TGV prox: 0 (the default) or s with 12 s^2 <= 1, the bound on ||K||^2 -- to 1e-6, so that the default rounded to float32 passes
int check_tgv_step(float step) {
  if (!(step >= 0.f) || !std::isfinite(step)) return fail(LMC_E_INVALID, "LMC_PRIOR_TGV: the step must be finite and >= 0 (0: the default 1 / sqrt(12)); got %g", (double)step);
  if (12.0 * (double)step * (double)step > 1.0 + 1e-6)
    return fail(LMC_E_INVALID, "LMC_PRIOR_TGV: step %g has 12 step^2 > 1: the primal-dual iteration needs step^2 ||K||^2 <= 1 and ||K||^2 < 12", (double)step);
  return LMC_OK;
}

int load_problem(const lmc_problem* p, Problem& q) {
  if (!p) return fail(LMC_E_INVALID, "lmc_problem is NULL");
  if (p->struct_size != sizeof(lmc_problem))
    return fail(LMC_E_INVALID, "lmc_problem.struct_size %u != %zu (ABI mismatch)", p->struct_size, sizeof(lmc_problem));
  if (p->H < 1 || p->W < 1 || (int64_t)p->H * p->W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad image size %dx%d", p->H, p->W);
  q.H = p->H; q.W = p->W;
  q.data_kind = p->data_kind;
  // Inside the library a public kind is the operator's kind plus the data term (every test on LMC_DATA_BLUR / IDENTITY / MASK / PSF serves every term; the
  // entry points without a form of a term refuse it: check_no_term, check_step_problem).  A large PSF is one operator kind of its own -- NOT LMC_DATA_BLUR,
  // whose taps stay empty: a path that was not taught about the PSF meets an unknown data kind, not a blur without taps.
  // no_mask: the term has no mask kind, and a caller that hands over a mask with the second plane would get it silently ignored -- say so instead
  struct KindMap { int op; lmc::DataTerm term; const char* no_mask; };
  static const char* const kWl2Mask = "(weighted Gaussian term) takes no mask_dev: there is no weighted mask kind, put the mask into the weights";
  static const char* const kHubMask = "(Huber data term) takes no mask_dev: there is no Huber mask kind, put the mask into the thresholds (delta = 0)";
  static const KindMap kKinds[LMC_DATA_SENSE + 1] = {
      {LMC_DATA_NONE, lmc::kTermL2, nullptr},      {LMC_DATA_IDENTITY, lmc::kTermL2, nullptr},  {LMC_DATA_BLUR, lmc::kTermL2, nullptr},   {LMC_DATA_MASK, lmc::kTermL2, nullptr},
      {LMC_DATA_IDENTITY, lmc::kTermPois, nullptr}, {LMC_DATA_BLUR, lmc::kTermPois, nullptr},    {LMC_DATA_MASK, lmc::kTermPois, nullptr},
      {LMC_DATA_IDENTITY, lmc::kTermWl2, kWl2Mask}, {LMC_DATA_BLUR, lmc::kTermWl2, kWl2Mask},
      {LMC_DATA_PSF, lmc::kTermL2, nullptr},        {LMC_DATA_PSF, lmc::kTermPois, nullptr},
      {LMC_DATA_PSF, lmc::kTermWl2, "(weighted Gaussian term) takes no mask_dev: put the mask into the weights"},
      {LMC_DATA_SPECTRAL, lmc::kTermL2, nullptr},
      {LMC_DATA_IDENTITY, lmc::kTermHub, kHubMask}, {LMC_DATA_BLUR, lmc::kTermHub, kHubMask},    {LMC_DATA_PSF, lmc::kTermHub, kHubMask},
      // (the Radon kinds take no mask for any term: the operator's case below says so)
      {LMC_DATA_RADON, lmc::kTermL2, nullptr},      {LMC_DATA_RADON, lmc::kTermPois, nullptr},   {LMC_DATA_RADON, lmc::kTermWl2, nullptr}, {LMC_DATA_RADON, lmc::kTermHub, nullptr},
      {LMC_DATA_SENSE, lmc::kTermL2, nullptr}};
  if (p->data_kind >= 0 && p->data_kind <= LMC_DATA_SENSE) {     // (any other kind: "unknown data_kind" below)
    const KindMap& k = kKinds[p->data_kind];
    const bool bad_mask = k.no_mask && p->mask_dev;
    const bool bad_geometry = k.op == LMC_DATA_PSF && (p->kh || p->kw || p->oy || p->ox);
    // (with both wrong the Huber PSF kind names the mask, the weighted PSF kind the geometry)
    if (bad_geometry && !(bad_mask && k.term == lmc::kTermHub))
      return fail(LMC_E_INVALID, "data_kind %d (large PSF) takes its geometry in the psf_* fields: kh = kw = oy = ox = 0", p->data_kind);
    if (bad_mask) return fail(LMC_E_INVALID, "data_kind %d %s", p->data_kind, k.no_mask);
    q.data_kind = k.op;
    q.term = k.term;
  }
  q.sigma_f = p->sigma_f;
  q.y = p->y_dev;
  q.mask = p->mask_dev;
  switch (q.data_kind) {
    case LMC_DATA_NONE: break;
    case LMC_DATA_IDENTITY:
      if (!p->y_dev) return fail(LMC_E_INVALID, "data term needs y_dev");
      break;
    case LMC_DATA_MASK:
      if (!p->y_dev || !p->mask_dev) return fail(LMC_E_INVALID, "mask data term needs y_dev and mask_dev");
      break;
    case LMC_DATA_BLUR: {
      if (!p->y_dev) return fail(LMC_E_INVALID, "data term needs y_dev");
      int rc = fill_taps(q.taps, p->h_host, p->kh, p->kw, p->oy, p->ox);
      if (rc) return rc;
      break;
    }
    case LMC_DATA_PSF: {
      if (!p->y_dev) return fail(LMC_E_INVALID, "data term needs y_dev");
      if (!p->h_host) return fail(LMC_E_INVALID, "PSF pointer (h_host) is NULL");
      if (p->psf_kh < 1 || p->psf_kw < 1 || p->psf_kh > lmc::kPsfMax || p->psf_kw > lmc::kPsfMax)
        return fail(LMC_E_INVALID, "PSF %dx%d outside 1..%d", p->psf_kh, p->psf_kw, lmc::kPsfMax);
      if (p->psf_oy >= p->psf_kh || p->psf_ox >= p->psf_kw)
        return fail(LMC_E_INVALID, "PSF offset (%d,%d) outside the kernel", p->psf_oy, p->psf_ox);
      if (p->psf_separable < 0 || p->psf_separable > 2) return fail(LMC_E_INVALID, "psf_separable must be 0 (auto), 1 (require) or 2 (forbid)");
      if (!lmc::psf_prepare(q.psf, p->h_host, p->psf_kh, p->psf_kw, p->psf_oy, p->psf_ox, p->psf_separable))
        return fail(LMC_E_INVALID, "psf_separable = 1 on a kernel that is no outer product to 2^-22 of every tap (lmc_psf_separable)");
      break;
    }
    case LMC_DATA_SPECTRAL:
      if (!p->y_dev) return fail(LMC_E_INVALID, "LMC_DATA_SPECTRAL needs y_dev: the [11][H][W / 2 + 1] planes of lmc_spectral_tables");
      if (p->mask_dev || p->h_host || p->kh || p->kw || p->oy || p->ox || p->psf_kh || p->psf_kw || p->psf_oy || p->psf_ox)
        return fail(LMC_E_INVALID, "LMC_DATA_SPECTRAL reads y_dev alone: mask_dev, h_host, kh, kw, oy, ox and the psf_* fields must be NULL / 0");
      if (!lmc::fft_shape_ok(p->H, p->W))
        return fail(LMC_E_UNSUPPORTED, "LMC_DATA_SPECTRAL: H and W must be powers of two in %d .. %d (got %dx%d)", lmc::kFftMin, lmc::kFftMax, p->H, p->W);
      q.fft.on = 1; q.fft.tab = p->y_dev;
      break;
    case LMC_DATA_RADON: {      // kh = n_angles, kw = n_det, h_host = the angles (include/lmc_atomi.h)
      if (!p->y_dev) return fail(LMC_E_INVALID, "data_kind %d (Radon operator) needs y_dev: the sinogram-shaped data", p->data_kind);
      if (p->mask_dev || p->oy || p->ox || p->psf_kh || p->psf_kw || p->psf_oy || p->psf_ox || p->psf_separable)
        return fail(LMC_E_INVALID, "data_kind %d (Radon operator) reads kh = n_angles, kw = n_det and h_host = the angles: mask_dev, oy, ox and the psf_* fields must be NULL / 0",
                    p->data_kind);
      if (!p->h_host) return fail(LMC_E_INVALID, "data_kind %d (Radon operator): h_host (the angles) is NULL", p->data_kind);
      if (p->kh < 1 || p->kh > lmc::kRadonMaxAngles) return fail(LMC_E_INVALID, "Radon operator: n_angles (kh) %d outside 1..%d", p->kh, lmc::kRadonMaxAngles);
      if (p->kw < 1 || p->kw > lmc::kRadonMaxDet) return fail(LMC_E_INVALID, "Radon operator: n_det (kw) %d outside 1..%d", p->kw, lmc::kRadonMaxDet);
      for (int a = 0; a < p->kh; ++a)
        if (!std::isfinite(p->h_host[a])) return fail(LMC_E_INVALID, "Radon operator: angle %d is not finite", a);
      if (p->H > lmc::kRadonMaxSide || p->W > lmc::kRadonMaxSide)
        return fail(LMC_E_UNSUPPORTED, "Radon operator: image sides up to %d (got %dx%d)", lmc::kRadonMaxSide, p->H, p->W);
      lmc::radon_prepare(q.radon, p->h_host, p->kh, p->kw);
      break;
    }
    case LMC_DATA_SENSE:      // kh = n_coils, y_dev = the [1 + 4 n_coils][H][W] descriptor (include/lmc_atomi.h)
      if (!p->y_dev) return fail(LMC_E_INVALID, "LMC_DATA_SENSE needs y_dev: the [1 + 4 n_coils][H][W] planes M, Re / Im S_c, Re / Im b_c");
      if (p->mask_dev || p->h_host || p->kw || p->oy || p->ox || p->psf_kh || p->psf_kw || p->psf_oy || p->psf_ox)
        return fail(LMC_E_INVALID, "LMC_DATA_SENSE reads y_dev and kh = n_coils alone: mask_dev, h_host, kw, oy, ox and the psf_* fields must be NULL / 0");
      if (p->kh < 1 || p->kh > lmc::kSenseMaxCoils) return fail(LMC_E_INVALID, "LMC_DATA_SENSE: n_coils (kh) %d outside 1..%d", p->kh, lmc::kSenseMaxCoils);
      if (!lmc::fft_shape_ok(p->H, p->W))
        return fail(LMC_E_UNSUPPORTED, "LMC_DATA_SENSE: H and W must be powers of two in %d .. %d (got %dx%d)", lmc::kFftMin, lmc::kFftMax, p->H, p->W);
      q.sense.on = 1; q.sense.n_coils = p->kh; q.sense.desc = p->y_dev;
      break;
    default: return fail(LMC_E_INVALID, "unknown data_kind %d", p->data_kind);
  }
  q.prior_kind = p->prior_kind;
  q.prior_sigma = p->prior_sigma;
  if (p->box_enable && (p->prior_kind == LMC_PRIOR_TV_ISO || p->prior_kind == LMC_PRIOR_TV_ANISO) && p->tv_niter == 0)
    return fail(LMC_E_INVALID, "box with a TV prior: the projection runs inside the dual iterations, tv_niter must be >= 1");
  switch (p->prior_kind) {
    case LMC_PRIOR_NONE: case LMC_PRIOR_L2: case LMC_PRIOR_L1: break;
    case LMC_PRIOR_EPROX:
      if (p->eprox_kind < 0 || p->eprox_kind > LMC_EPROX_LAPLACE_CONJ) return fail(LMC_E_INVALID, "unknown eprox_kind %d", p->eprox_kind);
      if (p->eprox_scale_mask < 0 || p->eprox_scale_mask > 3) return fail(LMC_E_INVALID, "eprox_scale_mask must be 0..3");
      if (!(p->eprox_p0 == p->eprox_p0) || !(p->eprox_p1 == p->eprox_p1)) return fail(LMC_E_INVALID, "eprox parameter is NaN");
      if (!eprox_params_ok(p->eprox_kind, p->eprox_p0, p->eprox_p1))
        return fail(LMC_E_INVALID, "eprox_kind %d: negative weight %g, %g", p->eprox_kind, (double)p->eprox_p0, (double)p->eprox_p1);
      q.eprox_kind = p->eprox_kind; q.eprox_mask = p->eprox_scale_mask; q.eprox_p0 = p->eprox_p0; q.eprox_p1 = p->eprox_p1;
      break;
    case LMC_PRIOR_HAAR_L1:
      if ((p->H & 7) || (p->W & 7)) return fail(LMC_E_UNSUPPORTED, "the Haar-l1 prior needs H and W to be multiples of 8 (got %dx%d)", p->H, p->W);
      break;
    case LMC_PRIOR_WAVELET_L1:      // tv_niter = levels, eprox_kind = p (include/lmc_atomi.h)
      if (p->eprox_kind < 1 || p->eprox_kind > lmc::kWaveletMaxP)
        return fail(LMC_E_INVALID, "LMC_PRIOR_WAVELET_L1: eprox_kind holds p, the vanishing moments of the filter, 1..%d (got %d)", lmc::kWaveletMaxP, p->eprox_kind);
      if (p->tv_niter < 1 || p->tv_niter > LMC_MAX_WAVELET_LEVELS)
        return fail(LMC_E_INVALID, "LMC_PRIOR_WAVELET_L1: tv_niter holds the levels of the transform, 1..%d (got %d)", LMC_MAX_WAVELET_LEVELS, p->tv_niter);
      if (!lmc::wavelet_shape_ok(p->H, p->W, p->eprox_kind, p->tv_niter))
        return fail(LMC_E_INVALID, "LMC_PRIOR_WAVELET_L1: a %dx%d image does not take %d levels of db%d: H and W must be multiples of 2^levels and "
                    "min(H, W) >> (levels - 1) >= 2p", p->H, p->W, p->tv_niter, p->eprox_kind);
      q.wav.on = 1; q.wav.p = p->eprox_kind; q.wav.levels = p->tv_niter;
      break;
    case LMC_PRIOR_TV_ANISO:
      // tv_niter = 0: the callers that never form the prox (ULPDA, lmc_energies); the entry points that do refuse it (check_step_problem)
      if (p->tv_niter == 0) break;
      [[fallthrough]];
    case LMC_PRIOR_TV_ISO:
      if (p->tv_niter < 1 || p->tv_niter > lmc::kMaxTvIters)
        return fail(LMC_E_UNSUPPORTED, "tv_niter %d outside 1..%d", p->tv_niter, lmc::kMaxTvIters);
      if (!(p->tv_rtol >= 0.f) || p->tv_rtol >= 1.f) return fail(LMC_E_INVALID, "tv_rtol must be in [0, 1)");
      q.tv_rtol = p->tv_rtol;
      q.tv_niter_asked = p->tv_niter;
      q.tv_niter = p->tv_niter - (p->tv_lagged_output ? 1 : 0);     // lagged: the iterate after tv_niter - 1 dual updates (0: prox = x)
      q.tv_step = p->tv_step > 0.f ? p->tv_step : 0.125f;
      if (p->tv_betas_host) std::memcpy(q.betas, p->tv_betas_host, sizeof(float) * p->tv_niter);
      else default_betas(q.betas, p->tv_niter);
      break;
    case LMC_PRIOR_VTV:
      return fail(LMC_E_UNSUPPORTED, "LMC_PRIOR_VTV (vectorial TV) acts on a multi-channel image: it is built for lmc_mch_create, lmc_vtv_prox and lmc_vtv_value only; "
                  "this entry point takes single-plane images");
    case LMC_PRIOR_TGV: {      // tv_niter = niter, eprox_p0 = alpha0, tv_step = s (include/lmc_atomi.h)
      if (p->tv_niter < 1 || p->tv_niter > LMC_MAX_TGV_ITERS)
        return fail(LMC_E_INVALID, "LMC_PRIOR_TGV: tv_niter holds the iterations of the prox, 1..%d (got %d)", LMC_MAX_TGV_ITERS, p->tv_niter);
      if (!std::isfinite(p->eprox_p0) || !(p->eprox_p0 > 0.f))
        return fail(LMC_E_INVALID, "LMC_PRIOR_TGV: eprox_p0 holds alpha0, the weight of the second-order term, finite and > 0 (got %g)", (double)p->eprox_p0);
      const int rc = check_tgv_step(p->tv_step);
      if (rc) return rc;
      if (p->tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "LMC_PRIOR_TGV with tv_rtol > 0: the prox has no early exit; it runs the fixed count tv_niter");
      if (p->tv_warm) return fail(LMC_E_UNSUPPORTED, "LMC_PRIOR_TGV with tv_warm: a primal-dual state carried across sampler iterations is not built");
      if (p->tv_lagged_output) return fail(LMC_E_UNSUPPORTED, "LMC_PRIOR_TGV with tv_lagged_output: the prox returns the iterate after tv_niter iterations");
      q.tgv_niter = p->tv_niter; q.tgv_alpha0 = p->eprox_p0; q.tgv_step = p->tv_step > 0.f ? p->tv_step : lmc::kTgvStep;
      break;
    }
    default: return fail(LMC_E_INVALID, "unknown prior_kind %d", p->prior_kind);
  }
  if (p->prior_kind != LMC_PRIOR_NONE && p->prior_kind != LMC_PRIOR_EPROX && !(p->prior_sigma >= 0.f)) return fail(LMC_E_INVALID, "prior_sigma must be >= 0");
  if (p->ncvx_kind != LMC_NCVX_NONE) {
    if (p->ncvx_kind != LMC_NCVX_MC_TV && p->ncvx_kind != LMC_NCVX_ME_TV && p->ncvx_kind != LMC_NCVX_MC_TV_ANISO && p->ncvx_kind != LMC_NCVX_ME_TV_ANISO)
      return fail(LMC_E_INVALID, "unknown ncvx_kind %d", p->ncvx_kind);
    if (!(p->ncvx_gamma > 0.f)) return fail(LMC_E_INVALID, "ncvx_gamma must be > 0");
    const bool me = p->ncvx_kind == LMC_NCVX_ME_TV || p->ncvx_kind == LMC_NCVX_ME_TV_ANISO;
    if (me && (p->ncvx_niter < 1 || p->ncvx_niter > lmc::kMaxTvIters))
      return fail(LMC_E_INVALID, "ncvx_niter %d outside 1..%d", p->ncvx_niter, lmc::kMaxTvIters);
    q.ncvx_kind = p->ncvx_kind; q.ncvx_lambda = p->ncvx_lambda; q.ncvx_gamma = p->ncvx_gamma;
    // anisotropic ME-TV: inside the library the ME-TV kind with the 1-D inner prox (every code path that adds the term's gradient serves both)
    if (p->ncvx_kind == LMC_NCVX_ME_TV_ANISO) { q.ncvx_kind = LMC_NCVX_ME_TV; q.ncvx_aniso = 1; }
    // anisotropic MC-TV: inside the library the same kind with a NEGATIVE gamma -- mc_tv_grad (lmc_device.h) and the energy kernels take
    // the sign as "component-wise weights 1 / max(|d|, gamma)" instead of the pixel norm; every MC-TV code path serves both
    if (p->ncvx_kind == LMC_NCVX_MC_TV_ANISO) { q.ncvx_kind = LMC_NCVX_MC_TV; q.ncvx_gamma = -p->ncvx_gamma; }
    q.ncvx_niter = p->ncvx_niter - ((me && p->tv_lagged_output) ? 1 : 0);
    if (me) {
      if (!(p->ncvx_rtol >= 0.f) || p->ncvx_rtol >= 1.f) return fail(LMC_E_INVALID, "ncvx_rtol must be in [0, 1)");
      q.ncvx_rtol = p->ncvx_rtol;
    }
  }
  if (p->tv_exit_path != 0 && p->tv_exit_path != 1) return fail(LMC_E_INVALID, "tv_exit_path must be 0 (device path where covered) or 1 (pass by pass)");
  q.tv_exit_path = p->tv_exit_path;
  if (p->iterations_per_launch < 0 || p->iterations_per_launch > 2) return fail(LMC_E_INVALID, "iterations_per_launch must be 0 (auto), 1 or 2");
  if (p->moments_overlap < -1 || p->moments_overlap > 1) return fail(LMC_E_INVALID, "moments_overlap must be 0 (auto), 1 (on) or -1 (off)");
  if (p->moments_bg_workgroups < 0 || p->graph_replay < 0 || p->graph_replay > 1) return fail(LMC_E_INVALID, "bad moments_bg_workgroups / graph_replay");
  q.iters_per_launch = p->iterations_per_launch; q.moments_overlap = p->moments_overlap;
  q.moments_bg_wgs = p->moments_bg_workgroups;   // (graph_replay: validated, no effect)
  {
    const char* e = getenv("LMC_CHEB_PAIR");
    const char* e2 = getenv("LMC_ITERS_PER_LAUNCH");
    const int ipl = q.iters_per_launch ? q.iters_per_launch : (e2 ? atoi(e2) : 0);
    q.cheb_pair = ipl == 1 ? 0 : (ipl == 2 ? 2 : (e ? atoi(e) : 1));
  }
  if (p->step_variant < 0 || p->step_variant > 8 || p->step_variant == 2)
    return fail(LMC_E_INVALID, "step_variant %d: 0 (library default), 1 tile, 3 split, 4 point, 5 block, 6 rows, 7 pipe, 8 pipe2", p->step_variant);
  q.variant = p->step_variant;
  if (p->prox_scale) {
    if (p->prior_kind != LMC_PRIOR_L2 && p->prior_kind != LMC_PRIOR_L1 && p->prior_kind != LMC_PRIOR_EPROX)
      return fail(LMC_E_UNSUPPORTED, "prox_scale (array-valued epsg) is built for the closed-form priors (l2, l1, prox.py closed forms) only");
    if (p->prox_scale_chain_stride < 0 || p->prox_scale_pixel_stride < 0) return fail(LMC_E_INVALID, "prox_scale strides must be >= 0");
    q.prox_scale = p->prox_scale; q.prox_scale_cs = p->prox_scale_chain_stride; q.prox_scale_ps = p->prox_scale_pixel_stride;
  }
  q.tv_warm = (p->tv_warm != 0 && p->prior_kind == LMC_PRIOR_TV_ISO) ? 1 : 0;
  q.tv_warm_asked = p->tv_warm != 0;
  if (!(p->implicit_tol == p->implicit_tol)) return fail(LMC_E_INVALID, "implicit_tol is NaN");
  q.implicit_tol = p->implicit_tol;
  if (p->box_enable) {
    if (p->box_enable != 1) return fail(LMC_E_INVALID, "box_enable must be 0 or 1 (got %d)", p->box_enable);
    if (!(p->box_lo == p->box_lo) || !(p->box_hi == p->box_hi)) return fail(LMC_E_INVALID, "box: a bound is NaN");
    if (!(p->box_lo < p->box_hi)) return fail(LMC_E_INVALID, "box: needs box_lo < box_hi (got [%g, %g])", (double)p->box_lo, (double)p->box_hi);
    if (p->prior_kind == LMC_PRIOR_HAAR_L1)
      return fail(LMC_E_UNSUPPORTED, "box with LMC_PRIOR_HAAR_L1: the prior is not separable in the pixels, so the clamp of its prox is not the prox of the sum");
    if (p->prior_kind == LMC_PRIOR_WAVELET_L1)
      return fail(LMC_E_UNSUPPORTED, "box with LMC_PRIOR_WAVELET_L1: the prior is not separable in the pixels, so the clamp of its prox is not the prox of the sum");
    const bool tv = p->prior_kind == LMC_PRIOR_TV_ISO || p->prior_kind == LMC_PRIOR_TV_ANISO;
    if (tv && p->tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "box with tv_rtol > 0: the early exit's objective is that of the unconstrained prox; use the fixed count, tv_rtol = 0");
    if (tv && p->tv_warm) return fail(LMC_E_UNSUPPORTED, "box with tv_warm: the warm-started dual has no box form");
    q.box = 1; q.box_lo = p->box_lo; q.box_hi = p->box_hi;
  }
  return LMC_OK;
}

// The entry points that have no box-constrained form refuse a problem that carries one.
int check_no_box(const Problem& q, const char* who, const char* why) {
  if (!q.box) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take a box constraint (lmc_problem.box_enable): %s", who, why);
}

// One row per DataTerm (lmc_host.h)
const TermInfo kTerms[lmc::kNumTerms] = {
    {},
    {"the Poisson data term", "LMC_DATA_POISSON_*", "has no Poisson form", "myula_step_pipe_pois_kernel", "myula_step_pipe_pois_box_kernel", "myula_step_tile_pois_kernel",
     "myula_step_tile_pois_box_kernel", "Poisson", "a pointwise data term"},
    {"the weighted Gaussian data term", "LMC_DATA_WL2_*", "has no weighted form", "myula_step_pipe_wl2_kernel", "myula_step_pipe_wl2_box_kernel", "myula_step_tile_wl2_kernel",
     "myula_step_tile_wl2_box_kernel", "weighted Gaussian", "the identity"},
    {"the Huber data term", "LMC_DATA_HUBER_*", "has no Huber form", "myula_step_pipe_hub_kernel", "myula_step_pipe_hub_box_kernel", "myula_step_tile_hub_kernel",
     "myula_step_tile_hub_box_kernel", "Huber", "the identity"}};

int check_no_term(const Problem& q, lmc::DataTerm term, const char* who, const char* why) {
  if (q.term != term || term == lmc::kTermL2) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take %s (%s): %s", who, kTerms[term].name, kTerms[term].label, why);
}

// The entry points that have no form of the large PSF refuse a problem that carries one.
int check_no_psf(const Problem& q, const char* who, const char* why) {
  if (!q.psf.on) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take a large PSF (LMC_DATA_PSF, LMC_DATA_POISSON_PSF, LMC_DATA_WL2_PSF, LMC_DATA_HUBER_PSF): %s", who, why);
}

// The entry points that have no form of the spectral data term refuse a problem that carries one.
int check_no_spectral(const Problem& q, const char* who, const char* why) {
  if (!q.fft.on) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take the spectral data term (LMC_DATA_SPECTRAL): %s", who, why);
}

// The entry points that have no form of the Radon operator refuse a problem that carries one.
int check_no_radon(const Problem& q, const char* who, const char* why) {
  if (!q.radon.on) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take the Radon operator (LMC_DATA_RADON, LMC_DATA_POISSON_RADON, LMC_DATA_WL2_RADON, LMC_DATA_HUBER_RADON): %s", who, why);
}

// The entry points that have no form of the multi-coil SENSE term refuse a problem that carries one.
int check_no_sense(const Problem& q, const char* who, const char* why) {
  if (!q.sense.on) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s does not take the multi-coil SENSE data term (LMC_DATA_SENSE): %s", who, why);
}

// The data terms with step kernels of their own, in the order their refusals are made: its name in the messages, what the warm-started dual lacks
// for it, and whether its step is a fused kernel of the term (the tiled kernel's and the full-width pipeline's instantiations: no Haar prior, variants
// 0, 1, 7) or splits into the term's launches around the step of a problem without a data term (every prior and variant of that problem).
// The rows of kTerms, then the large PSF, the spectral term, the Radon operator and the SENSE term.
struct DataTermRules { const char *name, *warm; bool own_kernels; };
constexpr int kNDataTerms = 5;
static int data_terms_of(const Problem& q, DataTermRules (&r)[kNDataTerms]) {
  int n = 0;
  if (q.term != lmc::kTermL2) r[n++] = {kTerms[q.term].name, kTerms[q.term].warm, true};
  if (q.psf.on) r[n++] = {"a large PSF", "is not built for it", false};
  if (q.fft.on) r[n++] = {"the spectral data term", "is not built for it", false};
  if (q.radon.on) r[n++] = {"the Radon operator", "is not built for it", false};
  if (q.sense.on) r[n++] = {"the multi-coil SENSE data term", "is not built for it", false};
  return n;
}

static int check_convex_term(const Problem& q, const DataTermRules& r) {
  if (q.ncvx_kind == LMC_NCVX_NONE) return LMC_OK;
  return fail(LMC_E_UNSUPPORTED, "%s has no non-convex form: ncvx_kind must be LMC_NCVX_NONE", r.name);
}

int check_convex_terms(const Problem& q) {
  DataTermRules terms[kNDataTerms];
  const int n = data_terms_of(q, terms);
  for (int i = 0; i < n; ++i) { const int rc = check_convex_term(q, terms[i]); if (rc) return rc; }
  return LMC_OK;
}

int check_step_problem(const Problem& q, float b) {
  // the anisotropic TV prior beyond load_problem: an iteration count, and none of the options that are built for the isotropic prior only
  if (q.prior_kind == LMC_PRIOR_TV_ANISO) {
    if (q.tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "tv_rtol > 0 (early exit of the prox) is not built for LMC_PRIOR_TV_ANISO: use the fixed-count prox, tv_rtol = 0");
    if (q.tv_warm_asked) return fail(LMC_E_UNSUPPORTED, "tv_warm (warm-started dual) is not built for LMC_PRIOR_TV_ANISO");
    if (b != 0.f && q.tv_niter_asked < 1)
      return fail(LMC_E_INVALID, "LMC_PRIOR_TV_ANISO: the prox needs tv_niter in 1..%d (got 0)", lmc::kMaxTvIters);
  }
  DataTermRules terms[kNDataTerms];
  const int n = data_terms_of(q, terms);
  const bool tv = q.prior_kind == LMC_PRIOR_TV_ISO || q.prior_kind == LMC_PRIOR_TV_ANISO;
  for (int i = 0; i < n; ++i) {
    const DataTermRules& r = terms[i];
    if (r.own_kernels && (q.psf.on || q.radon.on)) continue;     // (Poisson / weighted / Huber on a large PSF or the Radon operator: the operator's rules -- its step launch has no data term)
    const int rc = check_convex_term(q, r);
    if (rc) return rc;
    if (tv && q.tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "%s with tv_rtol > 0: the early exit of the TV prox is not built for it; use the fixed count, tv_rtol = 0", r.name);
    if (q.tv_warm_asked) return fail(LMC_E_UNSUPPORTED, "%s with tv_warm: the warm-started dual %s", r.name, r.warm);
    if (!r.own_kernels) continue;
    if (q.prior_kind == LMC_PRIOR_HAAR_L1) return fail(LMC_E_UNSUPPORTED, "%s with LMC_PRIOR_HAAR_L1 is not built", r.name);
    const int v = variant_of(q);
    if (v != 0 && v != 1 && v != 7)
      return fail(LMC_E_UNSUPPORTED, "step_variant %d has no form of %s: 0 (auto), 1 (tile) or 7 (pipe, where it covers the problem)", v, r.name);
  }
  return LMC_OK;
}

// StepArgs for: out = a*x - t*grad f + b*prox_{pt*g}(x) + s*xi
int make_step_args(const Problem& q, float a, float t, float b, float pt, float s, lmc::StepArgs& A) {
  std::memset(&A, 0, sizeof A);
  A.H = q.H; A.W = q.W;
  A.data_kind = (t == 0.f) ? LMC_DATA_NONE : q.data_kind;   // skip the stencil work if its weight is zero
  A.term = A.data_kind != LMC_DATA_NONE ? q.term : lmc::kTermL2;
  A.sigma_f = q.sigma_f;
  A.y = q.y; A.mask = q.mask;
  A.blur = q.taps;
  A.prior_kind = (b == 0.f) ? LMC_PRIOR_NONE : q.prior_kind;
  // the anisotropic TV prior: inside the library the TV kind plus a flag (every dispatch test on LMC_PRIOR_TV_ISO serves both; the kernels that
  // have no anisotropic form say "not covered" when the flag is set).  Problem::prior_kind stays as given (ULPDA, the energies).
  if (A.prior_kind == LMC_PRIOR_TV_ANISO) { A.prior_kind = LMC_PRIOR_TV_ISO; A.tv_aniso = 1; }
  if (A.prior_kind == LMC_PRIOR_TV_ISO && q.tv_niter == 0) { A.prior_kind = LMC_PRIOR_NONE; A.tv_aniso = 0; }   // lagged output of a 1-iteration prox: x itself
  if (A.prior_kind == LMC_PRIOR_HAAR_L1 || A.prior_kind == LMC_PRIOR_WAVELET_L1) A.prior_p0 = pt * q.prior_sigma;  // soft threshold of the detail coefficients
  if (A.prior_kind == LMC_PRIOR_TGV) {      // the radius of the first-order ball; a zero weight leaves the indicator of the box, or nothing
    const float lam1 = pt * q.prior_sigma;
    if (!(lam1 >= 0.f) || !std::isfinite(lam1)) return fail(LMC_E_INVALID, "TGV prox parameter must be finite and >= 0 (got %g)", (double)lam1);
    if (lam1 == 0.f) A.prior_kind = LMC_PRIOR_NONE;
    A.prior_p0 = lam1;
  }
  if (A.prior_kind == LMC_PRIOR_L2) A.prior_p0 = 1.f / (1.f + pt * q.prior_sigma);
  if (A.prior_kind == LMC_PRIOR_L1) A.prior_p0 = pt * q.prior_sigma;
  if (A.prior_kind == LMC_PRIOR_EPROX) {     // prox.py closed forms: the parameters the mask names scale with the prox parameter
    A.eprox_kind = q.eprox_kind;
    A.prior_p0 = (q.eprox_mask & 1) ? pt * q.eprox_p0 : q.eprox_p0;
    A.prior_p1 = (q.eprox_mask & 2) ? pt * q.eprox_p1 : q.eprox_p1;
  }
  if (A.prior_kind == LMC_PRIOR_TV_ISO) {
    const float gam = pt * q.prior_sigma;
    if (!(gam > 0.f)) return fail(LMC_E_INVALID, "TV prox parameter must be > 0 (got %g)", (double)gam);
    A.tv.niter = q.tv_niter;
    A.tv.gamma = gam;
    A.tv.c = q.tv_step / gam;
    std::memcpy(A.tv.betas, q.betas, sizeof(float) * q.tv_niter);
  }
  if (t != 0.f && q.ncvx_kind == LMC_NCVX_MC_TV) {
    A.ncvx_kind = q.ncvx_kind; A.ncvx_lambda = q.ncvx_lambda; A.ncvx_gamma = q.ncvx_gamma; A.ncvx_inv_gamma = 1.f / q.ncvx_gamma;
  }
  // LMC_NCVX_ME_TV: the caller runs me_tv_prox first and sets A.extra / A.extra_coef
  // box constraint: part of the prox, so a launch without a prox term (b = 0) carries none; a lagged 1-iteration TV prox (x itself) becomes the projection
  if (q.box && b != 0.f) { A.box = 1; A.box_lo = q.box_lo; A.box_hi = q.box_hi; }
  A.a = a; A.t = t; A.b = b; A.s = s;
  A.noise_mode = LMC_NOISE_NONE;
  return LMC_OK;
}

// Pointers that the configuration does not use are pointed at the input state (always valid for the
// index ranges the kernels form) so that no kernel ever holds a null pointer it could dereference.
void sanitize_pointers(lmc::StepArgs& A) {
  if (!A.y) A.y = A.x_in;
  if (!A.mask) A.mask = A.x_in;
  if (!A.noise) A.noise = A.x_in;
}

hipError_t Workspace::bind_psf(lmc::PsfOp& P, size_t n_resid, hipStream_t st) {
  hipError_t e = hipSuccess;
  if (!psf_tab) e = hipMalloc(&psf_tab, sizeof P.tab);
  if (e == hipSuccess && !psf_host) e = hipHostMalloc(&psf_host, sizeof P.tab);
  if (e == hipSuccess && !psf_ev) e = hipEventCreateWithFlags(&psf_ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  if (!psf_valid || std::memcmp(psf_host, P.tab, sizeof P.tab) != 0) {
    if (psf_valid) e = hipEventSynchronize(psf_ev);      // the previous upload has read the pinned copy
    psf_valid = false;
    if (e != hipSuccess) return e;
    std::memcpy(psf_host, P.tab, sizeof P.tab);
    e = hipMemcpyAsync(psf_tab, psf_host, sizeof P.tab, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(psf_ev, st);
    if (e != hipSuccess) return e;
    psf_valid = true;
  }
  e = resid.need(n_resid);
  P.tab_dev = psf_tab;
  P.resid = resid.p;
  return e;
}

hipError_t Workspace::bind_fft(lmc::FftOp& F, size_t n_spec, size_t n_part) {
  if (!fft_tw) {
    float tw[2 * lmc::kFftTw];
    lmc::fft_twiddles(tw);
    float* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof tw);
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, tw, sizeof tw, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return e; }
    fft_tw = d;
  }
  hipError_t e = fft_spec.need(n_spec);
  if (e == hipSuccess) e = fft_part.need(n_part);
  F.tw = reinterpret_cast<const float2*>(fft_tw);
  F.spec = reinterpret_cast<float2*>(fft_spec.p);
  F.part = fft_part.p;
  return e;
}

hipError_t Workspace::bind_sense(lmc::SenseOp& S, size_t n_spec, size_t n_g, size_t n_part) {
  lmc::FftOp F;
  hipError_t e = bind_fft(F, n_spec, n_part);
  if (e == hipSuccess) e = resid.need(n_g);
  S.tw = F.tw; S.spec = F.spec; S.part = F.part;
  S.g = resid.p;
  return e;
}

hipError_t Workspace::bind_radon(lmc::RadonOp& R, int H, int W, size_t n_resid, hipStream_t st) {
  const int na = R.n_angles;
  std::vector<int32_t> key(3 + (size_t)na);
  key[0] = H; key[1] = W; key[2] = R.n_det;
  std::memcpy(key.data() + 3, R.angles, sizeof(float) * na);
  hipError_t e = hipSuccess;
  if (!radon_ev) e = hipEventCreateWithFlags(&radon_ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  if (key != radon_key) {
    const size_t nt = lmc::radon_table_floats(na, H, W);
    if (!radon_key.empty()) e = hipEventSynchronize(radon_ev);      // the previous upload has read the pinned copy
    radon_key.clear();
    if (e != hipSuccess) return e;
    if (nt > radon_cap) {
      if (radon_tab) (void)hipFree(radon_tab);
      if (radon_host) (void)hipHostFree(radon_host);
      radon_tab = radon_host = nullptr; radon_cap = 0;
      e = hipMalloc(&radon_tab, sizeof(float) * nt);
      if (e == hipSuccess) e = hipHostMalloc(&radon_host, sizeof(float) * nt);
      if (e != hipSuccess) return e;
      radon_cap = nt;
    }
    lmc::radon_tables(R, H, W, radon_host);
    e = hipMemcpyAsync(radon_tab, radon_host, sizeof(float) * nt, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(radon_ev, st);
    if (e != hipSuccess) return e;
    radon_key = std::move(key);
  }
  e = resid.need(n_resid);
  R.tab_dev = radon_tab;
  R.resid = resid.p;
  return e;
}

hipError_t prepare(Workspace& ws, Problem& q, const lmc::StepArgs& probe, int64_t n_img, float pt, int what, hipStream_t st) {
  const size_t n = (size_t)n_img, npx = n * q.H * q.W;
  const bool step = what & kForStep, want_f = what & kForEnergyF, want_g = what & kForEnergyG;
  const bool tv = step && probe.prior_kind == LMC_PRIOR_TV_ISO;                       // a TV prox runs (either form; not the lagged output of one pass)
  const bool me = q.ncvx_kind == LMC_NCVX_ME_TV && ((step && probe.t != 0.f) || want_f);    // the inner prox of the ME-TV term runs
  size_t n_prox = 0, n_rtmp = 0, n_dbl = 0;
  hipError_t e = hipSuccess;
  auto need = [&e](auto& buf, size_t count) { if (e == hipSuccess) e = buf.need(count); };
  if (needs_tv_state(q) && (tv || me)) { need(ws.state[0], 4 * npx); need(ws.state[1], 4 * npx); }
  if (me) {
    need(ws.extra, npx);
    if (e == hipSuccess && q.ncvx_rtol > 0.f) e = ws.rt_me.need(n, q.ncvx_niter);
    n_dbl = Workspace::exit_doubles(n);      // the envelope's two sums; the exit scalars of the 1-D prox and of the pass-by-pass exit
    if (q.ncvx_rtol > 0.f && !q.ncvx_aniso && !me_tv_exit_on_device(q, n_img)) n_rtmp = npx;
  }
  // a prox that is a launch of its own ahead of the step: the transforms, the closed forms (scalar or array-valued epsg), the box of a separable prior
  if (step && (probe.prior_kind == LMC_PRIOR_HAAR_L1 || probe.prior_kind == LMC_PRIOR_WAVELET_L1 || probe.prior_kind == LMC_PRIOR_TGV ||
               probe.prior_kind == LMC_PRIOR_EPROX || q.prox_scale || (probe.box && probe.prior_kind != LMC_PRIOR_TV_ISO)))
    n_prox = npx;
  if (step && probe.prior_kind == LMC_PRIOR_TGV) {      // a chained TGV prox: its 11-plane state ping-pong
    const size_t ns = lmc::tgv_state_floats(n_img, q.H, q.W, q.tgv_niter);
    need(ws.state[0], ns); need(ws.state[1], ns);
  }
  ws.tv_exit = -1;
  if (tv && q.tv_rtol > 0.f) {     // the early exit of the TV prior's prox: 1 inside the fused launch, 0 the prox alone first, 2 pass by pass
    ws.tv_exit = tv_prior_rt_mode(q, probe, pt);
    if (e == hipSuccess && ws.tv_exit != 2) e = ws.rt_tv.need(n, q.tv_niter);
    if (ws.tv_exit != 1) n_prox = npx;
    if (ws.tv_exit == 2) { n_rtmp = npx; n_dbl = Workspace::exit_doubles(n); }
  }
  if (q.psf.on && ((step && probe.data_kind == LMC_DATA_PSF) || want_f)) {
    if (e == hipSuccess) e = ws.bind_psf(q.psf, step && probe.data_kind == LMC_DATA_PSF ? npx : 0, st);
    if (want_f) n_dbl = std::max(n_dbl, lmc::psf_energy_partials(n_img, q.H, q.W));
  }
  if (e == hipSuccess && q.fft.on && ((step && probe.data_kind == LMC_DATA_SPECTRAL) || want_f))
    e = ws.bind_fft(q.fft, lmc::fft_spec_floats(n_img, q.H, q.W), want_f ? lmc::fft_value_partials(n_img, q.H, q.W) : 0);
  if (q.radon.on && ((step && probe.data_kind == LMC_DATA_RADON) || want_f)) {
    const size_t n_resid = step && probe.data_kind == LMC_DATA_RADON ? n * q.radon.n_angles * q.radon.n_det : 0;
    if (e == hipSuccess) e = ws.bind_radon(q.radon, q.H, q.W, n_resid, st);
    if (want_f) n_dbl = std::max(n_dbl, lmc::radon_energy_partials(q.radon, n_img));
  }
  if (e == hipSuccess && q.sense.on && ((step && probe.data_kind == LMC_DATA_SENSE) || want_f))
    e = ws.bind_sense(q.sense, lmc::sense_spec_floats(n_img, q.H, q.W), step && probe.data_kind == LMC_DATA_SENSE ? npx : 0,
                      want_f ? lmc::sense_value_partials(n_img, q.H, q.W) : 0);
  if (q.wav.on && ((step && probe.prior_kind == LMC_PRIOR_WAVELET_L1) || want_g)) {
    need(ws.wav, lmc::wavelet_ws_floats(n_img, q.H, q.W));
    if (want_g) need(ws.wav_part, n * lmc::wavelet_partials(q.H, q.W, q.wav.levels));
    q.wav.ws = ws.wav.p;
    q.wav.part = ws.wav_part.p;
  }
  need(ws.prox, n_prox);
  need(ws.rtmp, n_rtmp);
  need(ws.dbl, n_dbl);
  return e;
}

// Library-wide DEFAULTS only (lmc_set_step_variant / lmc_set_cg_tolerance): every launch takes its variant and tolerance from the
// lmc_problem it was configured from (step_variant / implicit_tol) and falls back to these when that field is 0.
int g_variant = 0;  // 0 auto, 1 tile, (2: removed) 3 split, 4 point, 5 block, 6 rows, 7 pipe (one team), 8 pipe2 (two teams)
float g_cg_tol = 1e-6f;   // relative residual at which the inner solver stops (0: always cg_niter iterations)
int variant_of(const Problem& q) { return q.variant ? q.variant : g_variant; }
float tol_of(const Problem& q) { return q.implicit_tol > 0.f ? q.implicit_tol : (q.implicit_tol < 0.f ? 0.f : g_cg_tol); }

// Picks the step-kernel variant.  auto: the split streaming pipeline (two wave groups, 4 waves/SIMD) when
// it covers the configuration (W <= 512, separable blur <= 7x7, supported K), else the LDS-tiled kernel.
static hipError_t launch_step_nobox(const lmc::StepArgs& A_in, int variant, Workspace& ws, hipStream_t st, const char** name);

// The Poisson, weighted Gaussian and Huber data terms (kTerms).  The full-width pipeline's instantiations of the term where they cover the problem (isotropic
// TV, exactly 10 dual iterations, W > 128, separable blur or pointwise data term; auto and 7), the tiled kernel's everywhere else and for every other prior
// (auto and 1): TV (either form, box or not) and none / l2 / l1 run inside that kernel; a closed-form prior of prox.py and the box of a separable prior are
// formed by the elementwise launch before it and consumed as a ready-made prox.
bool term_pipe_covers(const lmc::StepArgs& A) { return A.term != lmc::kTermL2 && A.prior_kind == LMC_PRIOR_TV_ISO && lmc::pipe_links(A) == 1; }

static hipError_t launch_step_term(const lmc::StepArgs& A_in, int variant, Workspace& ws, hipStream_t st, const char** name) {
  const TermInfo& nm = kTerms[A_in.term];
  float *const state0 = ws.state[0].p, *const state1 = ws.state[1].p, *const pxbuf = ws.prox.p;
  if (variant != 0 && variant != 1 && variant != 7) return hipErrorInvalidConfiguration;
  if (variant != 1 && term_pipe_covers(A_in)) {
    if (name) *name = A_in.box ? nm.pipe_box : nm.pipe;
    return lmc::launch_step_pipe(A_in, st, nullptr, nullptr, 1);
  }
  if (variant == 7) return hipErrorInvalidConfiguration;
  if (A_in.ncvx_kind != LMC_NCVX_NONE || A_in.extra || A_in.prior_kind == LMC_PRIOR_HAAR_L1) return hipErrorInvalidConfiguration;
  lmc::StepArgs A = A_in;
  const bool tv = A.prior_kind == LMC_PRIOR_TV_ISO;
  if (!tv && !A.prox_ext && (A.box || A.prior_kind == LMC_PRIOR_EPROX)) {
    if (!pxbuf) return hipErrorInvalidConfiguration;
    hipError_t e = A.box ? lmc::launch_box_prox(A.prior_kind, A.eprox_kind, A.x_in, pxbuf, A.C, (int64_t)A.H * A.W, nullptr, 0, 0, 0.f, 0.f, A.prior_p0, A.prior_p1, 0,
                                                A.box_lo, A.box_hi, st)
                         : lmc::launch_eprox(A.eprox_kind, A.x_in, pxbuf, (int64_t)A.C * A.H * A.W, A.prior_p0, A.prior_p1, st);
    if (e != hipSuccess) return e;
    A.prox_ext = pxbuf;
  }
  if (!tv) { if (A.prox_ext) A.prior_kind = LMC_PRIOR_NONE; A.box = 0; }
  if (name) *name = A.box ? nm.tile_box : nm.tile;
  if (lmc::tile_needs_chunks(A)) {
    if (!state0 || !state1) return hipErrorInvalidConfiguration;
    return lmc::launch_step_tile_chunked(A, state0, state1, st);
  }
  return lmc::launch_step_tile(A, st);
}

// The box-constrained forms.  Separable priors: one elementwise launch forms clip(prox) into pxbuf, then the step of the variant asked for consumes it.
// TV priors: the pipe kernel's box instantiations (isotropic; auto, 7, 8) or the tile kernel's (either form; auto, 1); a forced variant without a box
// form is not covered.
// A data term that is launches of its own (a large PSF, the spectral term): the update as three steps.  residual(): the term's residual r at x_in into
// the operator's buffer; the step of the same arguments without a data term (t = 0: every prior, the box, the noise and the forced variant as they are
// there); adjoint(false, 0, c): x_out -= c Op^T r.  Without prox and noise the second step has nothing to do and adjoint(true, a, c) writes
// a x - c Op^T r under the kernel name `alone`.
template <class Residual, class Adjoint>
static hipError_t launch_step_around(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name, const char* alone,
                                     Residual residual, Adjoint adjoint) {
  if (A.ncvx_kind != LMC_NCVX_NONE || A.extra || A.tv_in || A.tv_out || A.f_out || A.g_out || A.rt_kc) return hipErrorInvalidConfiguration;
  hipError_t e = residual();
  if (e != hipSuccess) return e;
  const float coef = A.t * A.sigma_f;
  if (A.b == 0.f && A.s == 0.f) {
    if (name) *name = alone;
    return adjoint(true, A.a, coef);
  }
  lmc::StepArgs B = A;
  B.data_kind = LMC_DATA_NONE; B.t = 0.f; B.term = lmc::kTermL2;
  e = launch_step(B, variant, q, ws, st, name);      // (a wavelet prior: launch_step has formed its prox already, B carries it)
  if (e != hipSuccess) return e;
  return adjoint(false, 0.f, coef);
}

// A large PSF: r = rho(H x) into psf.resid, then H^T r.
static hipError_t launch_step_psf(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  const lmc::PsfOp& P = q.psf;
  if (!P.on || !P.tab_dev || !P.resid) return hipErrorInvalidConfiguration;
  const int rho = lmc::kPsfTermEpi[A.term].rho;
  return launch_step_around(A, variant, q, ws, st, name, "psf_conv_kernel",
      [&] { return lmc::launch_psf(P, 0, rho, A.x_in, P.resid, nullptr, A.y, A.C, A.H, A.W, 0.f, 0.f, st); },
      [&](bool alone, float a, float coef) {
        return lmc::launch_psf(P, 1, alone ? lmc::kPsfOverwrite : lmc::kPsfSub, P.resid, A.x_out, alone ? A.x_in : nullptr, nullptr, A.C, A.H, A.W, a, coef, st);
      });
}

// The spectral data term: the spectrum A xh - B of the gradient into fft.spec (row transform, then the column kernel with its functor between the two
// column transforms), then the row inverse.
static hipError_t launch_step_fft(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  const lmc::FftOp& F = q.fft;
  if (!F.on || !F.tab || !F.tw || !F.spec) return hipErrorInvalidConfiguration;
  return launch_step_around(A, variant, q, ws, st, name, "fft_rows_inv_kernel",
      [&] {
        const hipError_t e = lmc::launch_fft_rows_fwd(A.x_in, F.spec, F.tw, A.C, A.H, A.W, st);
        return e != hipSuccess ? e : lmc::launch_fft_cols(lmc::kFftGrad, F.spec, F.tab, F.tw, A.C, A.H, A.W, 0.f, st);
      },
      [&](bool alone, float a, float coef) {
        return lmc::launch_fft_rows_inv(alone ? lmc::kFftOverwrite : lmc::kFftSub, F.spec, A.x_out, alone ? A.x_in : nullptr, F.tw, A.C, A.H, A.W, a, coef, st);
      });
}

// The multi-coil SENSE term: the whole gradient image g into sense.g (three launches per coil through sense.spec), then the elementwise step 3.
static hipError_t launch_step_sense(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  const lmc::SenseOp& S = q.sense;
  if (!S.on || !S.desc || !S.tw || !S.spec || !S.g) return hipErrorInvalidConfiguration;
  const size_t n = (size_t)A.C * A.H * A.W;
  return launch_step_around(A, variant, q, ws, st, name, "sense_axpy_kernel",
      [&] { return lmc::launch_sense_gradient(S, A.x_in, A.C, A.H, A.W, st); },
      [&](bool alone, float a, float coef) { return lmc::launch_sense_axpy(alone, S.g, alone ? A.x_in : nullptr, A.x_out, n, a, coef, st); });
}

// The Radon operator: r = rho(A x) into radon.resid (a sinogram per chain), then A^T r.
static hipError_t launch_step_radon(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  const lmc::RadonOp& R = q.radon;
  if (!R.on || !R.tab_dev || !R.resid) return hipErrorInvalidConfiguration;
  const int rho = lmc::kRadonTermEpi[A.term].rho;
  return launch_step_around(A, variant, q, ws, st, name, "radon_adj_kernel",
      [&] { return lmc::launch_radon_forward(R, rho, A.x_in, R.resid, A.y, A.C, A.H, A.W, st); },
      [&](bool alone, float a, float coef) {
        return lmc::launch_radon_adjoint(R, alone ? lmc::kRadonOverwrite : lmc::kRadonSub, R.resid, A.x_out, alone ? A.x_in : nullptr, A.C, A.H, A.W, a, coef, st);
      });
}

hipError_t launch_step(const lmc::StepArgs& A_in, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  float *const state0 = ws.state[0].p, *const state1 = ws.state[1].p, *const pxbuf = ws.prox.p;
  if (A_in.prior_kind == LMC_PRIOR_WAVELET_L1) {
    // the route of LMC_PRIOR_HAAR_L1 in launch_step_nobox, taken before the data terms part ways: the prox into pxbuf, then the step of the same
    // problem without a prior, which consumes it as a ready-made prox -- on whatever kernel that problem gets
    if (!pxbuf || !q.wav.on || !q.wav.ws) return hipErrorInvalidConfiguration;
    hipError_t e = lmc::launch_wavelet_prox(A_in.x_in, pxbuf, A_in.C, A_in.H, A_in.W, q.wav.p, q.wav.levels, A_in.prior_p0, q.wav.ws, st);
    if (e != hipSuccess) return e;
    lmc::StepArgs A = A_in;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = pxbuf;
    return launch_step(A, variant, q, ws, st, name);
  }
  if (A_in.prior_kind == LMC_PRIOR_TGV) {
    // the same route: the primal-dual prox (with the box inside its iterations) into pxbuf, then the step of the same problem without prior and box
    if (!pxbuf) return hipErrorInvalidConfiguration;
    hipError_t e = lmc::launch_tgv_prox(A_in.x_in, pxbuf, nullptr, A_in.C, A_in.H, A_in.W, A_in.prior_p0, q.tgv_alpha0, q.tgv_step, q.tgv_niter, A_in.box,
                                        A_in.box_lo, A_in.box_hi, state0, state1, st);
    if (e != hipSuccess) return e == hipErrorInvalidValue ? hipErrorInvalidConfiguration : e;
    lmc::StepArgs A = A_in;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = pxbuf;
    A.box = 0;
    return launch_step(A, variant, q, ws, st, name);
  }
  if (A_in.data_kind == LMC_DATA_PSF) return launch_step_psf(A_in, variant, q, ws, st, name);
  if (A_in.data_kind == LMC_DATA_SPECTRAL) return launch_step_fft(A_in, variant, q, ws, st, name);
  if (A_in.data_kind == LMC_DATA_RADON) return launch_step_radon(A_in, variant, q, ws, st, name);
  if (A_in.data_kind == LMC_DATA_SENSE) return launch_step_sense(A_in, variant, q, ws, st, name);
  if (A_in.term != lmc::kTermL2) return launch_step_term(A_in, variant, ws, st, name);
  if (!A_in.box) return launch_step_nobox(A_in, variant, ws, st, name);
  lmc::StepArgs A = A_in;
  if (A.prior_kind != LMC_PRIOR_TV_ISO) {
    if (A.prior_kind == LMC_PRIOR_HAAR_L1 || !pxbuf) return hipErrorInvalidConfiguration;
    if (!A.prox_ext) {     // (a ready-made prox is clamped already: array-valued epsg)
      hipError_t e = lmc::launch_box_prox(A.prior_kind, A.eprox_kind, A.x_in, pxbuf, A.C, (int64_t)A.H * A.W, nullptr, 0, 0, 0.f, 0.f, A.prior_p0, A.prior_p1, 0,
                                          A.box_lo, A.box_hi, st);
      if (e != hipSuccess) return e;
      A.prox_ext = pxbuf;
    }
    A.prior_kind = LMC_PRIOR_NONE;
    A.box = 0;
    return launch_step_nobox(A, variant, ws, st, name);
  }
  const int v = variant;
  if (v == 0 || v == 7 || v == 8) {
    const int links = A.tv_aniso ? 0 : lmc::pipe_links(A);
    if (links == 1 || (links > 1 && state0 && state1 && v != 8)) {
      if (name) {       // the name of the kernel launch_step_pipe picks: two teams where covered unless one team is forced
        lmc::StepArgs T = A;
        const bool two = links == 1 && v != 7 && lmc::pipe_teams_covered(A, lmc::pipe_taps(T));
        *name = two ? "myula_step_pipe_box2_kernel" : "myula_step_pipe_box_kernel";
      }
      return lmc::launch_step_pipe(A, st, state0, state1, v == 7 ? 1 : v == 8 ? 2 : 0);
    }
  }
  if (v != 0 && v != 1) return hipErrorInvalidConfiguration;
  if (name) *name = "myula_step_tile_box_kernel";
  if (lmc::tile_needs_chunks(A)) {
    if (!state0 || !state1) return hipErrorInvalidConfiguration;
    return lmc::launch_step_tile_chunked(A, state0, state1, st);
  }
  return lmc::launch_step_tile(A, st);
}

static hipError_t launch_step_nobox(const lmc::StepArgs& A_in, int variant, Workspace& ws, hipStream_t st, const char** name) {
  float *const state0 = ws.state[0].p, *const state1 = ws.state[1].p, *const pxbuf = ws.prox.p;
  int v = variant;
  // no stencil in the data term and a prox local to 8 x 8 blocks (Haar-l1, l2, l1, none): the register-block kernel
  if ((v == 0 || v == 5) && lmc::block_supported(A_in)) {
    if (name) *name = "myula_step_block_kernel";
    return lmc::launch_step_block(A_in, st);
  }
  if ((v == 0 || v == 5) && A_in.ncvx_kind == LMC_NCVX_MC_TV) {
    // stencil-free data term + block-local prox + MC-TV term: the block kernel without the term, then one stencil
    // pass that adds t * lambda * A^T(A x / max(|A x|, gamma)) to its output
    lmc::StepArgs B = A_in;
    B.ncvx_kind = LMC_NCVX_NONE;
    if (lmc::block_supported(B)) {
      if (name) *name = "myula_step_block_kernel";
      hipError_t e = lmc::launch_step_block(B, st);
      if (e != hipSuccess) return e;
      return lmc::launch_mc_tv_add(A_in.x_in, A_in.x_out, A_in.C, A_in.H, A_in.W, A_in.t * A_in.ncvx_lambda, A_in.ncvx_gamma, st);
    }
  }
  if (v == 5) return hipErrorInvalidConfiguration;
  lmc::StepArgs A = A_in;
  if (A.prior_kind == LMC_PRIOR_HAAR_L1) {   // other data terms: the block-wavelet prox first, consumed by the fused step kernel
    if (!pxbuf) return hipErrorInvalidConfiguration;
    hipError_t e = lmc::launch_haar_prox(A.x_in, pxbuf, A.C, A.H, A.W, A.prior_p0, st);
    if (e != hipSuccess) return e;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = pxbuf;
  }
  // separable blur + closed-form prior (no TV pipeline): barrier-free row streaming, one wave per band of rows
  if ((v == 0 || v == 6) && lmc::rows_supported(A)) {
    if (name) *name = "myula_step_rows_kernel";
    return lmc::launch_step_rows(A, st);
  }
  if (v == 6) return hipErrorInvalidConfiguration;
  // TV K = 10 on a 264..512-wide image with a separable blur: the stage-parallel full-width pipeline (auto: its two-team layout where that
  // covers the configuration, else one team; 7: one team; 8: the two-team layout or nothing)
  if (v == 0 || v == 7 || v == 8) {
    const int links = lmc::pipe_links(A);
    if (links == 1 || (links > 1 && state0 && state1 && v != 8)) {
      if (name) *name = A.tv_aniso ? "myula_step_pipe_aniso_kernel" : "myula_step_pipe_kernel";
      return lmc::launch_step_pipe(A, st, state0, state1, v == 7 ? 1 : v == 8 ? 2 : 0);
    }
  }
  if (v == 7 || v == 8) return hipErrorInvalidConfiguration;
  // auto: split pipeline when it covers the configuration (W <= 512); for wider images the tiled kernels:
  // "point" for closed-form priors with a separable blur, else the general LDS-tiled kernel
  // a closed-form elementwise prior (LMC_PRIOR_EPROX) that reaches this point (a non-log-concave term, or a blur the row kernel does not cover): the split and
  // tiled kernels have no functor for it -- the point kernel evaluates it in place; where that does not cover the data term the prox is formed by one elementwise
  // launch and consumed as a ready-made prox.  (Round 3's configuration-matrix test found these combinations running with prox = identity.)
  if (A.prior_kind == LMC_PRIOR_EPROX) {
    if ((v == 0 || v == 4) && lmc::point_supported(A)) v = 4;
    else {
      if (!pxbuf) return hipErrorInvalidConfiguration;
      hipError_t e = lmc::launch_eprox(A.eprox_kind, A.x_in, pxbuf, (int64_t)A.C * A.H * A.W, A.prior_p0, A.prior_p1, st);
      if (e != hipSuccess) return e;
      A.prior_kind = LMC_PRIOR_NONE;
      A.prox_ext = pxbuf;
    }
  }
  if (v == 0) v = lmc::split_supported(A) ? 3 : (lmc::point_supported(A) ? 4 : 1);
  if (v == 4) {
    if (!lmc::point_supported(A)) return hipErrorInvalidConfiguration;
    if (name) *name = "myula_step_point_kernel";
    return lmc::launch_step_point(A, st);
  }
  if (v == 3) {
    if (!lmc::split_supported(A)) return hipErrorInvalidConfiguration;
    if (name) *name = "myula_step_split_kernel";
    return lmc::launch_step_split(A, st);
  }
  if (name) *name = "myula_step_tile_kernel";
  if (lmc::tile_needs_chunks(A)) {
    if (!state0 || !state1) return hipErrorInvalidConfiguration;
    return lmc::launch_step_tile_chunked(A, state0, state1, st);
  }
  return lmc::launch_step_tile(A, st);
}

}  // namespace lmc::host

using namespace lmc::host;

extern "C" {

float lmc_set_cg_tolerance(float tol) {
  const float prev = g_cg_tol;
  if (tol >= 0.f) g_cg_tol = tol;
  return prev;
}

int lmc_set_step_variant(int32_t variant) {
  if (variant < 0 || variant > 8 || variant == 2)
    return fail(LMC_E_INVALID, "variant must be 0 (auto), 1 (tile), 3 (split), 4 (point), 5 (block), 6 (rows), 7 (pipe) or 8 (pipe2); 2 (the one-group "
                "streaming kernel of ABI 1) was removed");
  const int prev = g_variant;
  g_variant = variant;
  return prev;
}

}  // extern "C"
