// The samplers behind lmc_sampler: create / destroy / state / step of MYULA, MYMALA, SK-ROCK and ULPDA, and the accessors of a handle (those of its
// accumulators: lmc_accum.hip).
#include <cmath>
#include <cstdlib>
#include <new>

#include "lmc_host.h"

using namespace lmc::host;

namespace {
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

// The checks of a sampler configuration that MYULA, MYMALA and ULPDA share, in the order the create calls make them: steps_ok / steps_msg are
// the sampler's own check of its step sizes, which comes after the chain ids.
template <class Cfg>
int check_config(const Cfg& cfg, bool steps_ok, const char* steps_msg) {
  if (cfg.n_chains < 1) return fail(LMC_E_INVALID, "n_chains must be >= 1");
  if (cfg.chain_offset < 0 || cfg.chain_offset + cfg.n_chains > 0xFFFFFFFFLL)
    return fail(LMC_E_INVALID, "global chain ids must fit 32 bits");
  if (!steps_ok) return fail(LMC_E_INVALID, "%s", steps_msg);
  if (cfg.noise_mode < LMC_NOISE_PHILOX || cfg.noise_mode > LMC_NOISE_NONE) return fail(LMC_E_INVALID, "bad noise_mode");
  return LMC_OK;
}

// The posterior-moment accumulators of a sampler created with moments on.
hipError_t alloc_moments(lmc_sampler* s) {
  return s->moments ? s->acc.alloc(s->C, s->chain_offset, s->prob.H, s->prob.W) : hipSuccess;
}

// A create call whose device allocation failed: the sampler goes, the status says why.
int alloc_failed(lmc_sampler* s, hipError_t e) {
  const int rc = fail(e == hipErrorOutOfMemory ? LMC_E_NOMEM : LMC_E_HIP, "sampler allocation failed: %s", hipGetErrorString(e));
  lmc_sampler_destroy(s);
  return rc;
}
}  // namespace

namespace lmc::host {
int rebuild_base(lmc_sampler* s) {
  // x <- (1 - tau/gamma) x - tau grad f(x) + (tau/gamma) prox_{epsg*gamma*g}(x) + sqrt(2 tau) xi   (algs.py:569)
  lmc::StepArgs A;
  const int rc = make_step_args(s->prob, 1.f - s->tau / s->gamma, s->tau, s->tau / s->gamma, s->epsg * s->gamma,
                                std::sqrt(2.f * s->tau), A);
  if (rc) return rc;
  s->base = A;
  s->base.C = s->C;
  s->base.noise_mode = s->noise_mode;
  s->base.key0 = (uint32_t)(s->seed & 0xFFFFFFFFu);
  s->base.key1 = (uint32_t)(s->seed >> 32);
  s->base.chain_offset = (uint32_t)s->chain_offset;
  return LMC_OK;
}

int check_weight_settable(const lmc_sampler* s) {
  if (s->kind == 2) return fail(LMC_E_UNSUPPORTED, "MYMALA caches the Metropolis energy of its state at the weight it was created with: the weight cannot change");
  if (s->kind == 1) return fail(LMC_E_UNSUPPORTED, "the prior weight of a ULPDA handle cannot change");
  if (s->prob.tv_warm) return fail(LMC_E_UNSUPPORTED, "tv_warm carries a dual that belongs to the weight it was formed with: the weight cannot change");
  if (s->prob.prox_scale) return fail(LMC_E_UNSUPPORTED, "prox_scale (array-valued epsg) carries the weights itself: the scalar weight cannot change");
  if (s->prob.box) return fail(LMC_E_UNSUPPORTED, "the handle carries a box constraint: the estimation of the weight rests on the homogeneity of g on the whole space (the d / k term), which does not hold on a bounded set");
  if (s->prob.prior_kind == LMC_PRIOR_NONE || s->prob.prior_kind == LMC_PRIOR_EPROX)
    return fail(LMC_E_UNSUPPORTED, "prior_kind %d has no weight prior_sigma", s->prob.prior_kind);
  if (s->prob.prior_kind == LMC_PRIOR_TGV)
    return fail(LMC_E_UNSUPPORTED, "the weight of the TGV prior (LMC_PRIOR_TGV) cannot be estimated or moved: its value g(x), the statistic of the estimator, is not built");
  return LMC_OK;
}

}  // namespace lmc::host

extern "C" {

int lmc_sampler_set_prior_sigma(lmc_sampler* s, float sigma) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  int rc = check_weight_settable(s);
  if (rc) return rc;
  if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(LMC_E_INVALID, "prior_sigma must be finite and > 0 (got %g)", (double)sigma);
  const float old = s->prob.prior_sigma;
  s->prob.prior_sigma = sigma;
  rc = rebuild_base(s);
  if (rc) s->prob.prior_sigma = old;     // s->base is untouched by a failed rebuild
  return rc;
}

// ---- sampler ---------------------------------------------------------------------------------

int lmc_myula_create(const lmc_myula_config* cfg, lmc_sampler** out) {
  if (!cfg || !out) return fail(LMC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(lmc_myula_config))
    return fail(LMC_E_INVALID, "lmc_myula_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(lmc_myula_config));
  int rc = check_config(*cfg, cfg->tau > 0.f && cfg->gamma > 0.f, "tau and gamma must be > 0");
  if (rc) return rc;
  if (cfg->moments && cfg->thin < 1) return fail(LMC_E_INVALID, "thin must be >= 1");
  lmc_sampler* s = new (std::nothrow) lmc_sampler();
  if (!s) return fail(LMC_E_NOMEM, "host allocation failed");
  rc = load_problem(&cfg->problem, s->prob);
  if (rc) { delete s; return rc; }
  rc = check_step_problem(s->prob, cfg->tau / cfg->gamma);
  if (rc) { delete s; return rc; }
  if (hipGetDevice(&s->device) != hipSuccess) { delete s; return fail(LMC_E_HIP, "hipGetDevice failed"); }
  s->C = cfg->n_chains;
  s->chain_offset = cfg->chain_offset;
  s->tau = cfg->tau; s->gamma = cfg->gamma; s->epsg = cfg->epsg;
  s->seed = cfg->seed;
  s->noise_mode = cfg->noise_mode;
  s->moments = cfg->moments; s->burn_in = cfg->burn_in; s->thin = cfg->thin < 1 ? 1 : cfg->thin;
  rc = rebuild_base(s);
  if (rc) { delete s; return rc; }
  // (a Huber term on a large PSF is left to the PSF's own rules here; the Poisson and weighted ones on a PSF are refused by this text)
  // (any term on the Radon operator: the operator's rules -- the forced variant selects the kernel of the middle launch, as for LMC_DATA_NONE)
  if (s->prob.term != lmc::kTermL2 && !(s->prob.term == lmc::kTermHub && s->prob.psf.on) && !s->prob.radon.on && variant_of(s->prob) == 7 && !term_pipe_covers(s->base)) {
    const TermInfo& t = kTerms[s->prob.term];
    delete s;
    return fail(LMC_E_UNSUPPORTED, "step_variant 7 (pipe) does not cover this %s problem: isotropic TV with 10 dual iterations (after tv_lagged_output), "
                "W > 128, separable blur of 5 or 7 taps or %s; use 0 (auto) or 1 (tile)", t.v7_name, t.v7_ops);
  }
  if (s->prob.tv_rtol > 0.f && s->base.prior_kind == LMC_PRIOR_TV_ISO && s->prob.tv_warm) { delete s; return fail(LMC_E_UNSUPPORTED, "tv_rtol > 0 and tv_warm exclude each other"); }
  const size_t n = (size_t)s->C * s->prob.H * s->prob.W;
  hipError_t e = s->own.alloc(&s->x[0], n, true);
  if (e == hipSuccess) e = s->own.alloc(&s->x[1], n, false);
  // every work buffer of the step and of the energies, here and never inside lmc_sampler_step; the PSF table is on the device when this call returns
  // (the caller's step stream need not order against the null stream)
  if (e == hipSuccess) e = prepare(s->ws, s->prob, s->base, s->C, s->epsg * s->gamma, kForStep | kForEnergies, nullptr);
  if (e == hipSuccess && s->ws.psf_ev) e = hipEventSynchronize(s->ws.psf_ev);
  if (e == hipSuccess && s->ws.radon_ev) e = hipEventSynchronize(s->ws.radon_ev);      // (the Radon tables, likewise)
  {   // launch policy: the lmc_problem fields, their environment variables where a field is 0 -- read here, once, never inside lmc_sampler_step
    const Problem& q = s->prob;
    const int ipl = q.iters_per_launch ? q.iters_per_launch : env_int("LMC_ITERS_PER_LAUNCH", 0);
    s->pol_pair = ipl == 1 ? 0 : (ipl == 2 ? 2 : env_int("LMC_ROWS_PAIR", 1));
    s->pol_blockpair = ipl == 1 ? 0 : (ipl == 2 ? 1 : (env_int("LMC_BLOCK_PAIR", 1) != 0));
    s->pol_overlap = q.moments_overlap ? q.moments_overlap : (getenv("LMC_MOMENTS_OVERLAP") ? (env_int("LMC_MOMENTS_OVERLAP", 0) ? 1 : -1) : 0);
    s->pol_bg_wgs = q.moments_bg_wgs > 0 ? q.moments_bg_wgs : env_int("LMC_MOMENTS_BG_WGS", -1);
    // One iteration per launch (the pair kernels have no form of it) wherever an iteration is more than the one fused launch:
    //   prox_scale, box, wav.on, TGV   the prox is a launch of its own before every step (array-valued epsg, the clamp, the wavelet transforms, the primal-dual prox)
    //   term                      the weighted Gaussian, the Huber and the Poisson data terms have kernels of their own, none of them a pair kernel
    //   psf.on, fft.on, radon.on, sense.on  the large PSF, the spectral data term, the Radon operator and the SENSE term are launches around the step
    if (q.prox_scale || q.box || q.wav.on || q.prior_kind == LMC_PRIOR_TGV || q.term != lmc::kTermL2 || q.psf.on || q.fft.on || q.radon.on || q.sense.on) { s->pol_pair = 0; s->pol_blockpair = 0; }
  }
  if (e == hipSuccess && s->prob.tv_warm) {
    lmc::StepArgs probe = s->base;
    probe.x_in = s->x[0];
    if (s->base.prior_kind != LMC_PRIOR_TV_ISO || !lmc::pipe_warm_supported(probe)) {
      lmc_sampler_destroy(s);
      return fail(LMC_E_UNSUPPORTED, "tv_warm: needs tv_niter in {1, 2, 3} (after tv_lagged_output) and the full-width pipeline kernel "
                  "(W > 128, W %% 4 == 0 (%% 8 above 256), separable blur <= 7 taps / pointwise / no data term)");
    }
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = s->own.alloc(&s->tvwarm[i], 2 * n, true);
  }
  if (e == hipSuccess) e = alloc_moments(s);
  if (e != hipSuccess) return alloc_failed(s, e);
  s->kernel_name = "(no step launched yet)";
  *out = s;
  return LMC_OK;
}

void lmc_sampler_destroy(lmc_sampler* s) {
  if (!s) return;
  DeviceGuard dg(s->device);
  if (s->side) { (void)hipStreamSynchronize(s->side); (void)hipStreamDestroy(s->side); }
  s->own.release();
  s->ws.release();
  s->acc.release();
  delete s;
}

int lmc_sampler_set_state(lmc_sampler* s, const float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  const size_t nbytes = sizeof(float) * (size_t)s->C * s->prob.H * s->prob.W;
  HIP_TRY(hipMemcpyAsync(s->x[s->cur], x_dev, nbytes, hipMemcpyDeviceToDevice, S(stream)));
  if (s->kind == 1) HIP_TRY(hipMemcpyAsync(s->xhat, x_dev, nbytes, hipMemcpyDeviceToDevice, S(stream)));   // xhat = x (algs.py:426)
  if (s->tvwarm[s->wcur]) HIP_TRY(hipMemsetAsync(s->tvwarm[s->wcur], 0, 2 * nbytes, S(stream)));           // a new start: zero dual
  s->mala_fresh = false;
  return LMC_OK;
}

int lmc_sampler_get_state(lmc_sampler* s, float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  const size_t nbytes = sizeof(float) * (size_t)s->C * s->prob.H * s->prob.W;
  HIP_TRY(hipMemcpyAsync(x_dev, s->x[s->cur], nbytes, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

static int ulpda_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st);
static int mymala_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st);
static int skrock_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st);

// f(x_c), g(x_c) of `x` ([C][H][W]) with the sampler's problem, in the sampler's workspace
static int sampler_energies_at(lmc_sampler* s, const float* x, double* f_out_dev, double* g_out_dev, hipStream_t st) {
  return problem_energies(s->prob, x, s->C, f_out_dev, g_out_dev, s->ws, st);
}

// an iterate the posterior-moment accumulators keep: after burn-in, every thin-th (none while lmc_sampler_sapg runs)
static bool kept(const lmc_sampler* s, int64_t it) { return s->moments && !s->suspend_moments && it >= s->burn_in && (it - s->burn_in) % s->thin == 0; }

// ME-TV: the inner prox of the Moreau-envelope term at A.x_in, which the fused step then takes as its extra gradient term
static int me_tv_extra(lmc_sampler* s, lmc::StepArgs& A, hipStream_t st) {
  if (s->prob.ncvx_kind != LMC_NCVX_ME_TV) return LMC_OK;
  int rc = me_tv_prox(s->prob, A.x_in, s->C, s->ws, st);
  if (rc) return rc;
  A.extra = s->ws.extra.p;
  A.extra_coef = -s->prob.ncvx_lambda / s->prob.ncvx_gamma;
  return LMC_OK;
}

// One launch with coefficients, noise mode and noise array of its own in place of the sampler's (an SK-ROCK stage); ev_begin / ev_end (nullable)
// are recorded around the step launch.
struct StepOverride {
  float a, t, b, s;
  int noise_mode;
  const float* noise;
  hipEvent_t ev_begin, ev_end;
};

// out = base update of `x_in` with the sampler's coefficients; noise_scale 0 gives the proposal mean m(x_in)
static int sampler_update(lmc_sampler* s, const float* x_in, float* x_out, bool with_noise, const float* noise, uint32_t iteration,
                          hipStream_t st, const char** kname, double* f_out = nullptr, double* g_out = nullptr, bool* fused = nullptr,
                          const StepOverride* ov = nullptr) {
  lmc::StepArgs A = s->base;
  if (fused) *fused = false;
  // (a weighted Gaussian or a Huber data term: its pipe kernels form no by-products -- the caller takes f and g from sampler_energies_at, as for strips)
  if (f_out && g_out && s->prob.term != lmc::kTermWl2 && s->prob.term != lmc::kTermHub && (variant_of(s->prob) == 0 || variant_of(s->prob) == 7) && s->prob.ncvx_kind == LMC_NCVX_NONE && s->prob.prior_kind == LMC_PRIOR_TV_ISO) {
    // The pipe kernel returns f(x_in), g(x_in) as by-products where one launch WITH them covers the problem: the probe carries the outputs, since
    // they narrow the coverage (no column strips, a blur only).  Elsewhere the launch below runs without them -- on whatever kernel covers the
    // update alone, the strips and the pointwise data terms of the pipe kernel included -- and the caller forms the energies itself.
    lmc::StepArgs probe = A;
    probe.x_in = x_in;
    probe.f_out = f_out; probe.g_out = g_out;
    if (lmc::pipe_supported(probe)) {
      HIP_TRY(hipMemsetAsync(f_out, 0, sizeof(double) * s->C, st));
      HIP_TRY(hipMemsetAsync(g_out, 0, sizeof(double) * s->C, st));
      A.f_out = f_out; A.g_out = g_out; A.g_scale = s->prob.prior_sigma;
      if (fused) *fused = true;
    }
  }
  A.x_in = x_in;
  A.x_out = x_out;
  A.iteration = iteration;
  A.noise = noise;
  if (!with_noise) { A.s = 0.f; A.noise_mode = LMC_NOISE_NONE; A.noise = nullptr; }
  if (ov) { A.a = ov->a; A.t = ov->t; A.b = ov->b; A.s = ov->s; A.noise_mode = ov->noise_mode; A.noise = ov->noise; }
  sanitize_pointers(A);
  int rc = me_tv_extra(s, A, st);   // inner prox of the Moreau-envelope term, then the fused step
  if (rc) return rc;
  if (ov && ov->ev_begin) HIP_TRY(hipEventRecord(ov->ev_begin, st));
  hipError_t e = launch_step(A, s->prob, s->ws, st, kname);
  if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "no step-kernel variant covers this configuration");
  HIP_TRY(e);
  if (ov && ov->ev_end) HIP_TRY(hipEventRecord(ov->ev_end, st));
  return LMC_OK;
}

// ---- MYULA steps ----------------------------------------------------------------------------------------------------------------
// Posterior-moment reductions of one lmc_sampler_step call.  A kept iterate is reduced in line on the caller's stream, or on the sampler's
// side stream under the launches that follow.  The side stream runs its batches in the order they were enqueued, so the pending batches form
// a queue and waiting for one waits for every earlier one.  Three rules order them against the launches:
//  - a launch that writes an array first waits for every pending batch that reads it, whatever that launch keeps;
//  - an in-line reduction first waits for every pending batch (the accumulators are shared);
//  - the call joins every pending batch before it returns: nothing is in flight between calls.
struct SideMoments {
  lmc_sampler* s;
  hipStream_t st;             // the caller's stream
  bool overlap;               // reductions may go to the side stream in this call
  int bg_wgs;                 // workgroups of a side-stream reduction
  const float* reads[kSideBatches][2] = {};   // by slot: the arrays the batch in that slot reads; its end event is s->side_ev[1 + slot]
  int head = 0, n = 0;                        // pending batches: slots head .. head + n - 1 (mod kSideBatches), oldest first

  hipError_t wait_through(int i) {            // the caller's stream waits for pending batch i (0 = the oldest), hence for batches 0 .. i
    const int slot = (head + i) % kSideBatches;
    head = (slot + 1) % kSideBatches;
    n -= i + 1;
    return hipStreamWaitEvent(st, s->side_ev[1 + slot], 0);
  }
  hipError_t before_write(const float* a, const float* b = nullptr) {   // the launch about to be enqueued writes a and b (b may be NULL)
    for (int i = n - 1; i >= 0; --i)
      for (const float* r : reads[(head + i) % kSideBatches])
        if (r && (r == a || r == b)) return wait_through(i);
    return hipSuccess;
  }
  hipError_t join() { return n ? wait_through(n - 1) : hipSuccess; }
  // the kept iterates a and b (either may be NULL) that the launch just enqueued wrote: into the accumulators, beside later launches or in line
  int keep(const float* a, const float* b, bool beside) {
    if (!a && !b) return LMC_OK;
    if (beside) {
      if (n == kSideBatches) HIP_TRY(wait_through(0));
      const int slot = (head + n) % kSideBatches;
      HIP_TRY(hipEventRecord(s->side_ev[0], st));
      HIP_TRY(hipStreamWaitEvent(s->side, s->side_ev[0], 0));
      for (const float* x : {a, b})
        if (x) HIP_TRY(s->acc.reduce_bg(x, bg_wgs, s->side));
      HIP_TRY(hipEventRecord(s->side_ev[1 + slot], s->side));
      reads[slot][0] = a;
      reads[slot][1] = b;
      ++n;
    } else {
      HIP_TRY(join());
      for (const float* x : {a, b})
        if (x) HIP_TRY(s->acc.reduce(x, st));
    }
    s->acc.count += (uint64_t)s->C * ((a ? 1 : 0) + (b ? 1 : 0));
    return LMC_OK;
  }
};

// The array of its own for a kept iterate in between whose reduction runs under the next launch (alternating by launch).
static hipError_t xmid_array(lmc_sampler* s, float** out) {
  float*& xm = s->xmid[s->last_launches & 1];
  const hipError_t e = xm ? hipSuccess : s->own.alloc(&xm, (size_t)s->C * s->prob.H * s->prob.W, false);
  *out = xm;
  return e;
}

// The launch helpers below return the iterations they ran (0: they do not cover the next ones) or a negative lmc_status.

// Two MYULA iterations per launch (lmc_step_rows_pair.hip) where that kernel covers the configuration and the launch is large enough for its
// long bands: x_{k+2} goes to a third array (neighbouring bands re-read x_k), x_{k+1} is stored only when the moment accumulators keep it.
// lmc_problem.iterations_per_launch / LMC_ROWS_PAIR: 0 = never, 2 = wherever covered (tests), default = where it pays (n_chains * H >= 2^17).
static int myula_rows_pair(lmc_sampler* s, SideMoments& m, int left) {
  if (!s->pol_pair || left < 2 || s->tvwarm[0] || s->ws.tv_exit == 2 || s->prob.ncvx_kind != LMC_NCVX_NONE ||
      (variant_of(s->prob) != 0 && variant_of(s->prob) != 6) || (s->pol_pair != 2 && (long long)s->C * s->prob.H < (1 << 17)))
    return 0;
  lmc::StepArgs A = s->base;
  A.x_in = s->x[s->cur];
  A.iteration = (uint32_t)s->iteration;
  A.noise = nullptr;
  sanitize_pointers(A);
  if (!lmc::rows_pair_supported(A)) return 0;
  if (!s->xspare) HIP_TRY(s->own.alloc(&s->xspare, (size_t)s->C * s->prob.H * s->prob.W, false));
  const bool keep_mid = kept(s, s->iteration), keep_out = kept(s, s->iteration + 1);
  float* mid = keep_mid ? s->x[s->cur ^ 1] : nullptr;
  if (keep_mid && m.overlap) HIP_TRY(xmid_array(s, &mid));
  HIP_TRY(m.before_write(s->xspare, mid));
  A.x_out = s->xspare;
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches], m.st));
  HIP_TRY(lmc::launch_step_rows_pair(A, mid, m.st));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches + 1], m.st));
  s->kernel_name = "myula_step_rows_pair_kernel";
  int rc = m.keep(mid, keep_out ? s->xspare : nullptr, m.overlap);
  if (rc) return rc;
  std::swap(s->x[s->cur], s->xspare);        // x[cur] = x_{k+2}; the array that held x_k is the spare now
  s->iteration += 2;
  ++s->last_launches;
  return 2;
}

// Two iterations per launch on the register-block kernel (Haar prior, stencil-free data term: BASELINE config 5): the update never leaves a
// thread's 8 x 8 block, so the second iteration runs on the block while it is on chip; x_{k+1} is written (in place, over x_k) only when the
// moment accumulators keep it.  LMC_BLOCK_PAIR=0 turns it off.  Same arithmetic, same noise: bit-identical to two launches.
static int myula_block_pair(lmc_sampler* s, SideMoments& m, int left) {
  if (!s->pol_blockpair || left < 2 || s->tvwarm[0] || s->ws.tv_exit == 2 || s->prob.ncvx_kind != LMC_NCVX_NONE ||
      (variant_of(s->prob) != 0 && variant_of(s->prob) != 5))
    return 0;
  lmc::StepArgs A = s->base;
  A.x_in = s->x[s->cur];
  A.x_out = s->x[s->cur ^ 1];
  A.iteration = (uint32_t)s->iteration;
  A.noise = nullptr;
  sanitize_pointers(A);
  if (!lmc::block_pair_supported(A)) return 0;
  // four iterations on chip when none of the three iterates in between is kept (moments off, burn-in, thinning by >= 4)
  const bool four = left >= 4 && !kept(s, s->iteration) && !kept(s, s->iteration + 1) && !kept(s, s->iteration + 2);
  const int nf = four ? 4 : 2;
  const bool keep_mid = !four && kept(s, s->iteration), keep_out = kept(s, s->iteration + nf - 1);
  A.fused_iters = nf;
  A.x_mid = keep_mid ? s->x[s->cur] : nullptr;              // in place over x_k (the update is block-local) ...
  if (keep_mid && m.overlap) HIP_TRY(xmid_array(s, &A.x_mid));   // ... unless its reduction runs under the next launch, which writes x_{k+3} there
  HIP_TRY(m.before_write(A.x_out, A.x_mid));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches], m.st));
  HIP_TRY(lmc::launch_step_block(A, m.st));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches + 1], m.st));
  s->kernel_name = four ? "myula_step_block_kernel(4 iterations)" : "myula_step_block_kernel(2 iterations)";
  int rc = m.keep(A.x_mid, keep_out ? A.x_out : nullptr, m.overlap);
  if (rc) return rc;
  s->cur ^= 1;
  s->iteration += nf;
  ++s->last_launches;
  return nf;
}

// One iteration per launch: every configuration, and the only path for injected noise, the ME-TV term, the warm-started TV prox, the early
// exits of the TV prox and array-valued epsg.  `last`: the call's last iteration, whose reduction runs in line.
static int myula_single(lmc_sampler* s, SideMoments& m, const float* noise, bool last) {
  hipStream_t st = m.st;
  lmc::StepArgs A = s->base;
  A.x_in = s->x[s->cur];
  A.x_out = s->x[s->cur ^ 1];
  A.iteration = (uint32_t)s->iteration;
  A.noise = noise;
  sanitize_pointers(A);
  int rc = me_tv_extra(s, A, st);   // inner prox of the Moreau-envelope term, then the fused step
  if (rc) return rc;
  HIP_TRY(m.before_write(A.x_out));
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches], st));
  const char* kname = nullptr;
  hipError_t e;
  bool stepped = false;
  if (s->ws.tv_exit == 0 || s->ws.tv_exit == 1) {   // early exit of the TV prox decided on the device: inside the fused launch, or the prox alone first
    rc = tv_prior_rt(s->prob, s->epsg * s->gamma, A, s->ws, st);
    if (rc < 0) return rc;
    if (rc == 2) return fail(LMC_E_STATE, "the device-side early exit no longer covers this sampler");
    if (rc == 1) { stepped = true; kname = "myula_step_pipe_kernel(per-chain exit)"; }
  }
  if (s->ws.tv_exit == 2) {   // early-exit TV prox first (exact pass-by-pass path), consumed as a ready-made prox
    rc = tv_prox_rtol(s->prob, s->epsg * s->gamma, A.x_in, s->ws.prox.p, s->C, s->ws, st);
    if (rc) return rc;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = s->ws.prox.p;
  }
  if (s->prob.prox_scale && A.prior_kind != LMC_PRIOR_NONE) {   // array-valued epsg: prox_{epsg[c,i] gamma g} first, consumed as a ready-made prox
    const Problem& q = s->prob;
    if (A.box)     // the same launch with the clamp
      HIP_TRY(lmc::launch_box_prox(q.prior_kind, q.eprox_kind, A.x_in, s->ws.prox.p, s->C, (int64_t)q.H * q.W, q.prox_scale, q.prox_scale_cs, q.prox_scale_ps,
                                   s->epsg * s->gamma, q.prior_sigma, q.eprox_p0, q.eprox_p1, q.eprox_mask, A.box_lo, A.box_hi, st));
    else
    HIP_TRY(lmc::launch_prior_prox_scaled(q.prior_kind, q.eprox_kind, A.x_in, s->ws.prox.p, s->C, (int64_t)q.H * q.W, q.prox_scale, q.prox_scale_cs, q.prox_scale_ps,
                                          s->epsg * s->gamma, q.prior_sigma, q.eprox_p0, q.eprox_p1, q.eprox_mask, st));
    A.box = 0;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = s->ws.prox.p;
  }
  if (stepped) {
    e = hipSuccess;
  } else if (s->tvwarm[0]) {     // warm-started TV prox: the dual of the previous iteration in, this iteration's out
    A.tv_in = s->tvwarm[s->wcur];
    A.tv_out = s->tvwarm[s->wcur ^ 1];
    e = lmc::launch_step_pipe_warm(A, st);
    kname = "myula_step_pipe_kernel(warm)";
    s->wcur ^= 1;
  } else {
    e = launch_step(A, s->prob, s->ws, st, &kname);
  }
  if (e == hipErrorInvalidConfiguration)
    return fail(LMC_E_UNSUPPORTED, s->base.box ? "step_variant %d has no box-constrained form of this prior (TV: auto, 1 tile, 7 / 8 pipe where the pipe covers the problem)"
                                               : "no step-kernel variant covers this configuration", variant_of(s->prob));
  HIP_TRY(e);
  if (kname) s->kernel_name = kname;
  if (s->timing) HIP_TRY(hipEventRecord(s->ev[2 * s->last_launches + 1], st));
  s->cur ^= 1;
  if (kept(s, s->iteration)) {
    // beside the next launch unless the step kernel is a single launch of an HBM-heavy closed-form-prior kernel at full size: the two then share the memory
    // system and the reduction outlasts the kernel whatever its workgroup count (blur + l2, 512 x 512 x 1024: in line 0.714 ms per iteration, beside it 0.73-0.83)
    const bool beside = m.overlap && !last &&
                        (s->pol_overlap > 0 || s->base.prior_kind == LMC_PRIOR_TV_ISO || (long long)s->C * s->prob.H * s->prob.W <= (1LL << 25));
    rc = m.keep(s->x[s->cur], nullptr, beside);
    if (rc) return rc;
  }
  ++s->iteration;
  ++s->last_launches;
  return 1;
}

static int myula_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st) {
  const size_t per_iter = (size_t)s->C * s->prob.H * s->prob.W;
  s->timed = false;
  s->last_launches = 0;
  if (n_iters == 0) return LMC_OK;
  if (s->timing) {  // one event pair per step-kernel launch: moment reductions stay outside the brackets
    while ((int)s->ev.size() < 2 * n_iters) {
      hipEvent_t e;
      HIP_TRY(s->own.event(&e, hipEventDefault));
      s->ev.push_back(e);
    }
  }
  // Moment reductions on the side stream under the following launches (lmc_problem.moments_overlap / LMC_MOMENTS_OVERLAP): on at every size --
  // what bench.py's `value` measures -- and off while the launches are being event-timed (lmc_sampler_enable_timing: the roofline leg wants the
  // step kernel alone).  BASELINE config 2 (256 x 256 x 128): the 15 us reduction is 40 % of a serial iteration, 40.2 -> 35.9 us per iteration
  // with 128 background workgroups.  Headline size: the reduction under the step kernel costs that kernel 6 % (1.76 -> 1.89 ms per launch) and
  // saves its own 0.22 ms -- 1.976 -> 1.90-1.92 ms per iteration with 256 workgroups (16: 3.19, 64: 2.07, 128: 1.92, 256: 1.90, 512: 1.94,
  // 1024: 1.98 ms; too few and the reduction outlasts the step kernel).  Re-measured under the two-team kernel (four 112-VGPR waves per SIMD, one 64-VGPR wave
  // fits beside them): 128 / 192 / 256 / 384 / 512 workgroups of 256 threads: 1.725 / 1.729 / 1.709 / 1.710 / 1.771 ms per step; one-wave workgroups and a chain
  // unroll of 2 or 8 instead of 4 are equal at equal wave counts, never better: 256 stays.
  // (lmc_problem.moments_bg_workgroups / LMC_MOMENTS_BG_WGS: fixed at creation)
  const bool overlap = !s->timing && s->pol_overlap >= 0 && s->moments && !s->suspend_moments && n_iters > 1;
  const int bg_wgs = s->pol_bg_wgs >= 0 ? s->pol_bg_wgs : ((long long)per_iter <= (1LL << 25) ? 128 : 256);   // 0: the full-speed kernel
  if (overlap && !s->side) {
    int prio_least = 0, prio_greatest = 0;     // lowest priority: the step kernel's workgroups go first
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIP_TRY(hipStreamCreateWithPriority(&s->side, hipStreamNonBlocking, prio_least));
    for (hipEvent_t& e : s->side_ev) HIP_TRY(s->own.event(&e, hipEventDisableTiming));
  }
  SideMoments m{s, st, overlap, bg_wgs};
  for (int k = 0; k < n_iters;) {
    int done = 0;
    if (!noise_dev) done = myula_rows_pair(s, m, n_iters - k);        // the pair launches draw Philox noise
    if (!noise_dev && !done) done = myula_block_pair(s, m, n_iters - k);
    if (!done) done = myula_single(s, m, noise_dev ? noise_dev + (size_t)k * per_iter : nullptr, k + 1 == n_iters);
    if (done < 0) {
      (void)m.join();
      return done;
    }
    k += done;
  }
  HIP_TRY(m.join());   // everything this call enqueued is ordered before whatever the caller enqueues next
  s->timed = s->timing;
  return LMC_OK;
}

int lmc_sampler_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (n_iters < 0) return fail(LMC_E_INVALID, "n_iters < 0");
  if (s->noise_mode == LMC_NOISE_INJECTED && !noise_dev && n_iters > 0)
    return fail(LMC_E_INVALID, "noise_mode is INJECTED but noise_dev is NULL");
  if (s->noise_mode != LMC_NOISE_INJECTED && noise_dev)
    return fail(LMC_E_INVALID, "noise_dev given but noise_mode is not INJECTED");
  if (s->iteration + n_iters > 0xFFFFFFFFLL) return fail(LMC_E_STATE, "iteration counter would exceed 32 bits");
  if (s->kind == 3) return skrock_step(s, n_iters, noise_dev, S(stream));
  if (s->kind == 2) return mymala_step(s, n_iters, noise_dev, S(stream));
  if (s->kind == 1) return ulpda_step(s, n_iters, noise_dev, S(stream));
  return myula_step(s, n_iters, noise_dev, S(stream));
}

// ---- MYMALA: Metropolis-adjusted MYULA at image scale (generalises prox_lmc.py:134-158) -------------------------------
int lmc_mymala_create(const lmc_myula_config* cfg, lmc_sampler** out) {
  if (cfg && out && cfg->struct_size == sizeof(lmc_myula_config) && cfg->problem.data_kind == LMC_DATA_SPECTRAL) {      // (before any buffer exists)
    *out = nullptr;
    return fail(LMC_E_UNSUPPORTED, "MYMALA does not take the spectral data term (LMC_DATA_SPECTRAL): its Metropolis ratio is pinned for the fused step and its "
                "energy by-products, which the three-launch spectral step does not form; use MYULA or SK-ROCK");
  }
  if (cfg && out && cfg->struct_size == sizeof(lmc_myula_config) && cfg->problem.data_kind >= LMC_DATA_RADON && cfg->problem.data_kind <= LMC_DATA_HUBER_RADON) {
    *out = nullptr;
    return fail(LMC_E_UNSUPPORTED, "MYMALA does not take the Radon operator (LMC_DATA_RADON, LMC_DATA_POISSON_RADON, LMC_DATA_WL2_RADON, LMC_DATA_HUBER_RADON): its "
                "Metropolis ratio is pinned for the fused step and its energy by-products, which the three-launch Radon step does not form; use MYULA or SK-ROCK");
  }
  if (cfg && out && cfg->struct_size == sizeof(lmc_myula_config) && cfg->problem.data_kind == LMC_DATA_SENSE) {
    *out = nullptr;
    return fail(LMC_E_UNSUPPORTED, "MYMALA does not take the multi-coil SENSE data term (LMC_DATA_SENSE): its Metropolis ratio is pinned for the fused step and its "
                "energy by-products, which the coil-by-coil SENSE step does not form; use MYULA or SK-ROCK");
  }
  if (cfg && out && cfg->struct_size == sizeof(lmc_myula_config) && cfg->problem.prior_kind == LMC_PRIOR_TGV) {
    *out = nullptr;
    return fail(LMC_E_UNSUPPORTED, "MYMALA does not take the TGV prior (LMC_PRIOR_TGV): its value g(x) is a minimisation over the auxiliary field and is not built, "
                "so the Metropolis target exp(-f - epsg g) cannot be evaluated; use MYULA or SK-ROCK");
  }
  int rc = lmc_myula_create(cfg, out);
  if (rc) return rc;
  lmc_sampler* s = *out;
  *out = nullptr;
  if (s->tvwarm[0]) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "MYMALA needs a proposal mean that is a function of x alone: tv_warm is not allowed"); }
  if (s->ws.tv_exit >= 0) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "MYMALA with tv_rtol > 0 is not built (use the fixed-count prox, tv_rtol = 0)"); }
  if (s->prob.prox_scale) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "MYMALA takes a scalar epsg (the reference's array-valued epsg is MYULA's, algs.py:509)"); }
  if (s->prob.psf.on) { const lmc::host::Problem q = s->prob; lmc_sampler_destroy(s); return check_no_psf(q, "MYMALA", "its Metropolis ratio is pinned for the fused step and its energy by-products, which the three-launch PSF step does not form; use MYULA or SK-ROCK"); }
  if (s->prob.term == lmc::kTermPois) { const lmc::host::Problem q = s->prob; lmc_sampler_destroy(s); return check_no_term(q, lmc::kTermPois, "MYMALA", "its Metropolis ratio needs the energy by-products of the step, which the Poisson kernels do not form; use MYULA or SK-ROCK"); }
  if (s->prob.box) { const lmc::host::Problem q = s->prob; lmc_sampler_destroy(s); return check_no_box(q, "MYMALA", "its target would be +infinity outside the box, where MYULA's proposals land; use MYULA"); }
  if (s->prob.prior_kind == LMC_PRIOR_EPROX) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "MYMALA does not take a closed-form prior (LMC_PRIOR_EPROX): the prior has a prox and no value g(x), so its Metropolis target exp(-f - epsg g) is undefined; use MYULA"); }
  s->kind = 2;
  const size_t n = (size_t)s->C * s->prob.H * s->prob.W;
  hipError_t e = s->own.alloc(&s->mx, n, false);
  if (e == hipSuccess) e = s->own.alloc(&s->xp, n, false);
  if (e == hipSuccess) e = s->own.alloc(&s->mxp, n, false);
  if (e == hipSuccess) e = s->own.alloc(&s->mala_d, 6 * (size_t)s->C, true);
  if (e == hipSuccess) e = s->own.alloc(&s->flag, (size_t)s->C, false);
  if (e == hipSuccess) e = s->own.alloc(&s->nacc, (size_t)s->C, true);
  if (e != hipSuccess) return alloc_failed(s, e);
  *out = s;
  return LMC_OK;
}

static int mymala_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st) {
  const size_t img = (size_t)s->prob.H * s->prob.W, per_iter = (size_t)s->C * img;
  const int C = s->C;
  double *U = s->mala_d, *fp = U + C, *gp = U + 2 * C, *d1 = U + 3 * C, *d2 = U + 4 * C, *la = U + 5 * C;
  float* x = s->x[s->cur];
  s->timed = false;
  s->last_launches = 0;
  const char* kname = nullptr;
  if (!s->mala_fresh && n_iters > 0) {   // m(x) and U(x) = f(x) + g(x) of the current state (after create / set_state)
    bool fused = false;
    int rc = sampler_update(s, x, s->mx, false, nullptr, (uint32_t)s->iteration, st, &kname, fp, gp, &fused);
    if (rc) return rc;
    if (!fused) rc = sampler_energies_at(s, x, fp, gp, st);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d1, 0, sizeof(double) * C, st));
    HIP_TRY(lmc::launch_axpy_env(fp, gp, d1, C, -s->epsg, 1.f, st));    // fp += epsg * gp  (f -= (-epsg) * (g + d1/2) with d1 = 0): U = f + epsg g, the
                                                                        // potential MYULA's drift is built from (algs.py:569, 582)
    HIP_TRY(hipMemcpyAsync(U, fp, sizeof(double) * C, hipMemcpyDeviceToDevice, st));
    s->mala_fresh = true;
  }
  for (int k = 0; k < n_iters; ++k) {
    const float* xi = noise_dev ? noise_dev + (size_t)k * per_iter : s->xi;
    if (s->noise_mode == LMC_NOISE_PHILOX) {   // x' = m(x) + s xi with the Philox field drawn inside the proposal kernel, and ||x' - m(x)||^2
      HIP_TRY(lmc::mala_propose_philox(s->mx, s->xp, C, s->prob.H, s->prob.W, s->base.s, s->base.key0, s->base.key1, (uint32_t)s->iteration,
                                       s->base.chain_offset, d1, st));
    } else if (s->noise_mode == LMC_NOISE_NONE) {   // deterministic proposal x' = m(x): d1 = 0
      HIP_TRY(hipMemcpyAsync(s->xp, s->mx, sizeof(float) * per_iter, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemsetAsync(d1, 0, sizeof(double) * C, st));
    } else {
      HIP_TRY(lmc::mala_propose(s->mx, xi, s->xp, C, img, s->base.s, d1, st));          // x' and ||x' - m(x)||^2
    }
    bool fused = false;
    int rc = sampler_update(s, s->xp, s->mxp, false, nullptr, (uint32_t)s->iteration, st, &kname, fp, gp, &fused);   // m(x') [+ f, g]
    if (rc) return rc;
    if (!fused) rc = sampler_energies_at(s, s->xp, fp, gp, st);                           // f(x'), g(x')
    if (rc) return rc;
    HIP_TRY(lmc::launch_sqdiff(x, s->mxp, C, img, d2, st));                               // ||x - m(x')||^2
    HIP_TRY(lmc::mala_accept(C, U, fp, gp, s->epsg, d1, d2, s->tau, s->base.key0, s->base.key1, (uint32_t)s->iteration, s->base.chain_offset,
                             s->flag, s->nacc, la, st));
    // accepted chains: x <- x', m(x) <- m(x').  (The other direction -- keep the proposal buffers and give the rejected chains their old
    // state back -- was measured: 3.0 instead of 3.7 ms at 98 % acceptance, but 3.7 instead of 3.0 ms at 48 %; the choice would have to
    // follow the acceptance rate, which the host does not see without a synchronisation.)
    HIP_TRY(lmc::mala_select(s->flag, x, s->mx, s->xp, s->mxp, C, img, 1, st));
    if (kept(s, s->iteration)) {
      HIP_TRY(s->acc.reduce(x, st));
      s->acc.count += (uint64_t)C;
    }
    ++s->iteration;
  }
  if (kname) s->kernel_name = kname;
  return LMC_OK;
}

int lmc_sampler_get_acceptance(lmc_sampler* s, uint64_t* accepted_dev, double* last_log_alpha_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (s->kind != 2) return fail(LMC_E_STATE, "not a MYMALA sampler");
  if (accepted_dev) HIP_TRY(hipMemcpyAsync(accepted_dev, s->nacc, sizeof(uint64_t) * (size_t)s->C, hipMemcpyDeviceToDevice, S(stream)));
  if (last_log_alpha_dev)
    HIP_TRY(hipMemcpyAsync(last_log_alpha_dev, s->mala_d + 5 * (size_t)s->C, sizeof(double) * (size_t)s->C, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

// ---- SK-ROCK: s stages of the MYULA drift per iteration, each one launch of the fused step kernel (definition: lmc_atomi.h) -----------------
int lmc_skrock_coefficients(int32_t n_stages, double eta, double* mu, double* nu, double* kappa, double* step_factor) {
  if (n_stages < 2 || n_stages > LMC_MAX_SKROCK_STAGES) return fail(LMC_E_INVALID, "n_stages must be 2 .. %d (got %d)", LMC_MAX_SKROCK_STAGES, n_stages);
  if (!std::isfinite(eta) || !(eta > 0.0)) return fail(LMC_E_INVALID, "eta must be finite and > 0");
  const int s = n_stages;
  const double w0 = 1.0 + eta / ((double)s * s);
  double T[LMC_MAX_SKROCK_STAGES + 1], dT[LMC_MAX_SKROCK_STAGES + 1];     // T_j(w0), T_j'(w0): T_j = 2 w0 T_{j-1} - T_{j-2}, differentiated for T_j'
  T[0] = 1.0; T[1] = w0; dT[0] = 0.0; dT[1] = 1.0;
  for (int j = 2; j <= s; ++j) {
    T[j] = 2.0 * w0 * T[j - 1] - T[j - 2];
    dT[j] = 2.0 * T[j - 1] + 2.0 * w0 * dT[j - 1] - dT[j - 2];
  }
  const double w1 = T[s] / dT[s];
  for (int j = 1; j <= s; ++j) {
    if (mu) mu[j - 1] = j == 1 ? w1 / w0 : 2.0 * w1 * T[j - 1] / T[j];
    if (nu) nu[j - 1] = j == 1 ? s * w1 / 2.0 : 2.0 * w0 * T[j - 1] / T[j];
    if (kappa) kappa[j - 1] = j == 1 ? s * w1 / w0 : -T[j - 2] / T[j];
  }
  if (step_factor) *step_factor = (s - 0.5) * (s - 0.5) * (2.0 - 4.0 * eta / 3.0) - 1.5;
  return LMC_OK;
}

int lmc_skrock_create(const lmc_myula_config* cfg, int32_t n_stages, float eta, lmc_sampler** out) {
  if (!out) return fail(LMC_E_INVALID, "NULL argument");
  *out = nullptr;
  double mu[LMC_MAX_SKROCK_STAGES], nu[LMC_MAX_SKROCK_STAGES], kappa[LMC_MAX_SKROCK_STAGES];
  int rc = lmc_skrock_coefficients(n_stages, (double)eta, mu, nu, kappa, nullptr);
  if (rc) return rc;
  rc = lmc_myula_create(cfg, out);
  if (rc) return rc;
  lmc_sampler* s = *out;
  *out = nullptr;
  // every stage is a launch of the fused step kernel with coefficients of its own: what MYULA runs outside that launch has no stage form
  if (s->tvwarm[0]) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "SK-ROCK evaluates the drift at s different points per iteration: tv_warm (a dual carried between evaluations) is not allowed"); }
  if (s->ws.tv_exit >= 0) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "SK-ROCK with tv_rtol > 0 is not built (use the fixed-count prox, tv_rtol = 0)"); }
  if (s->prob.prox_scale) { lmc_sampler_destroy(s); return fail(LMC_E_UNSUPPORTED, "SK-ROCK takes a scalar epsg (array-valued epsg is MYULA's)"); }
  if (s->prob.box) { const lmc::host::Problem q = s->prob; lmc_sampler_destroy(s); return check_no_box(q, "SK-ROCK", "its stability bound is derived for the unconstrained Moreau-Yosida envelope; use MYULA"); }
  s->kind = 3;
  s->sk_stages = n_stages;
  for (int j = 0; j < n_stages; ++j) { s->sk_mu[j] = mu[j]; s->sk_nu[j] = nu[j]; s->sk_kappa[j] = kappa[j]; }
  const hipError_t e = s->own.alloc(&s->xspare, (size_t)s->C * s->prob.H * s->prob.W, false);   // the third array of the stage rotation
  if (e != hipSuccess) return alloc_failed(s, e);
  *out = s;
  return LMC_OK;
}

// One iteration = n_stages launches of the step kernel over three rotating arrays (x_in = K_{j-1}, noise = K_{j-2}, x_out = K_j, always
// distinct), after one streaming launch that forms the perturbed point of stage 1 in the array stage 1 does not write.
static int skrock_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st) {
  const size_t per_iter = (size_t)s->C * s->prob.H * s->prob.W;
  const int ns = s->sk_stages;
  const double delta = s->tau, dg = delta / (double)s->gamma, q = std::sqrt(2.0 * delta);
  s->timed = false;
  s->last_launches = 0;
  if (n_iters == 0) return LMC_OK;
  if (s->timing) {   // one event pair per stage launch; the perturbation launch and the reductions stay outside
    if ((long long)n_iters * ns > (1 << 24)) return fail(LMC_E_INVALID, "too many stage launches to time in one call");
    while (s->ev.size() < (size_t)2 * n_iters * ns) {
      hipEvent_t e;
      HIP_TRY(s->own.event(&e, hipEventDefault));
      s->ev.push_back(e);
    }
  }
  const char* kname = nullptr;
  for (int k = 0; k < n_iters; ++k) {
    float* X = s->x[s->cur];            // K_0
    float* Yb = s->x[s->cur ^ 1];       // the perturbed point, then K_2
    float* K1 = s->xspare;
    const uint32_t it = (uint32_t)s->iteration;
    const float* Z = noise_dev ? noise_dev + (size_t)k * per_iter : nullptr;
    const bool noisy = s->noise_mode != LMC_NOISE_NONE;
    const float* in1 = X;
    if (noisy) {   // Y = X + nu_1 q Z
      const float coef = (float)(s->sk_nu[0] * q);
      if (s->noise_mode == LMC_NOISE_PHILOX)
        HIP_TRY(lmc::launch_skrock_perturb_philox(X, Yb, s->C, s->prob.H, s->prob.W, coef, s->base.key0, s->base.key1, it, s->base.chain_offset, st));
      else
        HIP_TRY(lmc::launch_skrock_perturb(X, Z, Yb, per_iter, coef, st));
      in1 = Yb;
    }
    const float* prev2 = X;      // K_{j-2}
    const float* prev1 = nullptr;   // K_{j-1}
    float* free_buf = Yb;        // the array stage j writes, for j >= 2
    for (int j = 1; j <= ns; ++j) {
      const double mu = s->sk_mu[j - 1], nu = s->sk_nu[j - 1], kappa = s->sk_kappa[j - 1];
      StepOverride ov{};
      ov.t = (float)(mu * delta);
      ov.b = (float)(mu * dg);
      if (j == 1) {   // K_1 = Y - mu_1 delta/gamma (Y - prox(Y)) - mu_1 delta grad f(Y) + (kappa_1 - nu_1) q Z
        ov.a = (float)(1.0 - mu * dg);
        ov.s = noisy ? (float)((kappa - nu) * q) : 0.f;
        ov.noise_mode = s->noise_mode;
        ov.noise = Z;
      } else {        // K_j = nu_j K_{j-1} + mu_j delta drift(K_{j-1}) + kappa_j K_{j-2}
        ov.a = (float)(nu - mu * dg);
        ov.s = (float)kappa;
        ov.noise_mode = LMC_NOISE_INJECTED;
        ov.noise = prev2;
      }
      if (s->timing) { ov.ev_begin = s->ev[2 * s->last_launches]; ov.ev_end = s->ev[2 * s->last_launches + 1]; }
      const float* xin = j == 1 ? in1 : prev1;
      float* xout = j == 1 ? K1 : free_buf;
      int rc = sampler_update(s, xin, xout, true, nullptr, it, st, &kname, nullptr, nullptr, nullptr, &ov);
      if (rc) return rc;
      ++s->last_launches;
      if (j >= 2) {      // the array that held K_{j-2} is free now
        free_buf = const_cast<float*>(prev2);
        prev2 = prev1;
      }
      prev1 = xout;
    }
    // K_s becomes the public state; the other two arrays are the spares of the next iteration
    float* Ks = const_cast<float*>(prev1);
    float* all[3] = {X, Yb, K1};
    float* rest[2];
    int nr = 0;
    for (float* b : all) if (b != Ks) rest[nr++] = b;
    s->x[s->cur] = Ks;
    s->x[s->cur ^ 1] = rest[0];
    s->xspare = rest[1];
    if (kept(s, s->iteration)) {
      HIP_TRY(s->acc.reduce(Ks, st));
      s->acc.count += (uint64_t)s->C;
    }
    ++s->iteration;
  }
  if (kname) s->kernel_name = kname;
  s->timed = s->timing;
  return LMC_OK;
}

int lmc_sampler_enable_timing(lmc_sampler* s, int32_t on) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  s->timing = on != 0;
  s->timed = false;
  return LMC_OK;
}

// ---- ULPDA ---------------------------------------------------------------------------------------

static int ulpda_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, hipStream_t st) {
  const int H = s->prob.H, W = s->prob.W;
  const int64_t C = s->C;
  const size_t per_iter = (size_t)C * H * W;
  const int iso = s->prob.prior_kind == LMC_PRIOR_TV_ISO;
  s->timed = false;
  s->last_launches = 0;
  bool used_pairs = false;
  for (int k = 0; k < n_iters; ++k) {
    float* x = s->x[s->cur];
    const float ts = s->tau * s->prob.sigma_f;
    // pre-step of L2_ncvx_tv.prox: with a blur the right-hand side also takes tau sigma H^T b; the pointwise solves add their tau sigma m b themselves
    const float* htb_nc = s->prob.data_kind == LMC_DATA_BLUR ? s->htb : s->prob.y;
    const float ts_nc = s->prob.data_kind == LMC_DATA_BLUR ? ts : 0.f;
    if (s->gfirst)   // y <- proxdual(y + mu A xhat)   (algs.py:436)
      HIP_TRY(lmc::ulpda_dual_update(s->xhat, s->ydual, C, H, W, s->mu, s->prob.prior_sigma, iso, st));
    // v = x - tau (A^T y + z) [+ tau sigma H^T b]      (algs.py:437-440 / 443-446)
    if (s->prob.ncvx_kind == LMC_NCVX_MC_TV) {   // L2_ncvx_tv.prox pre-step (algs.py:213-217), then + tau sigma H^T b (:225)
      HIP_TRY(lmc::ulpda_rhs(x, s->ydual, s->z, nullptr, s->ctmp, C, H, W, s->tau, ts, st));
      HIP_TRY(lmc::ulpda_ncvx_rhs(s->ctmp, htb_nc, s->rhs, C, H, W, s->tau * s->prob.ncvx_lambda, s->prob.ncvx_gamma, ts_nc, st));
    } else if (s->prob.ncvx_kind == LMC_NCVX_ME_TV) {   // x += tau*lamda/gamma (x - prox_{gamma TV}(x))  (algs.py:221-223)
      HIP_TRY(lmc::ulpda_rhs(x, s->ydual, s->z, nullptr, s->ctmp, C, H, W, s->tau, ts, st));
      int rc = me_tv_prox(s->prob, s->ctmp, C, s->ws, st);
      if (rc) return rc;
      HIP_TRY(lmc::ulpda_me_rhs(s->ctmp, s->ws.extra.p, htb_nc, s->rhs, C, H, W, s->tau * s->prob.ncvx_lambda / s->prob.ncvx_gamma, ts_nc, st));
    } else {
      HIP_TRY(lmc::ulpda_rhs(x, s->ydual, s->z, s->prob.data_kind == LMC_DATA_BLUR ? s->htb : nullptr, s->rhs, C, H, W, s->tau, ts, st));
    }
    const float* u = s->rhs;
    if (s->prob.data_kind == LMC_DATA_BLUR) {
      if (!s->warm) HIP_TRY(hipMemsetAsync(s->uw, 0, sizeof(float) * per_iter, st));
      float* where = s->uw;
      { int rc = cg_solve_fused(s->prob, ts, s->uw, s->rhs, s->cr, s->cp, s->cq, s->scal, C, s->cg_niter, s->zero_y, st, s->uw2, &where); if (rc) return rc; }
      if (where != s->uw) { s->uw2 = s->uw; s->uw = where; used_pairs = true; }       // the pair launches deliver the solution in the other array
      u = s->uw;
    } else if (s->prob.data_kind != LMC_DATA_NONE) {
      HIP_TRY(lmc::ulpda_pointwise_prox(s->rhs, s->uw, s->prob.y, s->prob.mask, C, H, W, ts, s->prob.data_kind, st));
      u = s->uw;
    }
    // x <- u + sqrt(2 tau) xi ; xhat <- x + theta (x - x_old)     (algs.py:440-441 / 446-447)
    if (s->noise_mode == LMC_NOISE_PHILOX && (W & 3) == 0) {     // the Philox field is drawn inside the pass
      HIP_TRY(lmc::ulpda_finish_philox(x, s->xhat, u, C, H, W, std::sqrt(2.f * s->tau), s->theta, s->base.key0, s->base.key1,
                                       (uint32_t)s->iteration, s->base.chain_offset, st));
    } else {
      const float* xi = nullptr;
      if (s->noise_mode == LMC_NOISE_INJECTED) xi = noise_dev + (size_t)k * per_iter;
      else if (s->noise_mode == LMC_NOISE_PHILOX) {
        HIP_TRY(lmc::launch_noise(s->xi, (int)C, H, W, s->base.key0, s->base.key1, (uint32_t)s->iteration, s->base.chain_offset, st));
        xi = s->xi;
      }
      HIP_TRY(lmc::ulpda_finish(x, s->xhat, u, xi, C, H, W, std::sqrt(2.f * s->tau), s->theta, st));
    }
    if (!s->gfirst)  // (algs.py:448)
      HIP_TRY(lmc::ulpda_dual_update(s->xhat, s->ydual, C, H, W, s->mu, s->prob.prior_sigma, iso, st));
    if (kept(s, s->iteration)) {
      HIP_TRY(s->acc.reduce(x, st));
      s->acc.count += (uint64_t)s->C;
    }
    ++s->iteration;
  }
  s->kernel_name = used_pairs ? "ulpda (multi-kernel, chebyshev pairs)" : "ulpda (multi-kernel)";
  return LMC_OK;
}

int lmc_ulpda_create(const lmc_ulpda_config* cfg, lmc_sampler** out) {
  if (!cfg || !out) return fail(LMC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(lmc_ulpda_config))
    return fail(LMC_E_INVALID, "lmc_ulpda_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(lmc_ulpda_config));
  int rc = check_config(*cfg, cfg->tau > 0.f && cfg->mu > 0.f, "tau and mu must be > 0");
  if (rc) return rc;
  if (cfg->problem.prior_kind == LMC_PRIOR_TGV)
    return fail(LMC_E_UNSUPPORTED, "ULPDA does not take the TGV prior (LMC_PRIOR_TGV): it needs g o A with a dual prox in closed form (L21 or L1 on the gradient); "
                "the TGV prox is an inner primal-dual loop of its own; use MYULA or SK-ROCK");
  if (cfg->problem.prior_kind != LMC_PRIOR_TV_ISO && cfg->problem.prior_kind != LMC_PRIOR_TV_ANISO)
    return fail(LMC_E_UNSUPPORTED, "ULPDA needs g o A with g = L21 (LMC_PRIOR_TV_ISO) or L1 (LMC_PRIOR_TV_ANISO)");
  if (!(cfg->problem.prior_sigma > 0.f)) return fail(LMC_E_INVALID, "prior_sigma (dual ball radius) must be > 0");
  if (cfg->problem.data_kind == LMC_DATA_BLUR && cfg->cg_niter < 1) return fail(LMC_E_INVALID, "cg_niter must be >= 1");
  if (cfg->problem.ncvx_kind != LMC_NCVX_NONE && cfg->problem.data_kind == LMC_DATA_NONE)
    return fail(LMC_E_UNSUPPORTED, "the non-convex term belongs to a data term (blur, identity or mask)");
  lmc_sampler* s = new (std::nothrow) lmc_sampler();
  if (!s) return fail(LMC_E_NOMEM, "host allocation failed");
  lmc_problem pr = cfg->problem;
  if (pr.prior_kind == LMC_PRIOR_TV_ISO && pr.tv_niter < 1) pr.tv_niter = 1;   // unused by ULPDA; keeps the loader happy
  rc = load_problem(&pr, s->prob);
  if (!rc) rc = check_no_radon(s->prob, "ULPDA", "its primal step is the implicit step of f, (I + tau sigma_f A^T A)^{-1}, which is not built for the Radon operator; use MYULA");
  if (!rc) rc = check_no_term(s->prob, lmc::kTermHub, "ULPDA", "its primal step is the implicit step of f, which has no closed form for the Huber loss under an operator; use MYULA");
  if (!rc) rc = check_no_term(s->prob, lmc::kTermWl2, "ULPDA", "its primal step is the implicit step of f, (I + tau sigma_f Op^T W Op)^{-1}, which is not built; use MYULA");
  if (!rc) rc = check_no_term(s->prob, lmc::kTermPois, "ULPDA", "its primal step is the implicit step of f, which has no closed form for the Poisson likelihood; use MYULA");
  if (!rc) rc = check_no_psf(s->prob, "ULPDA", "its primal step is the implicit step of f, (I + tau sigma_f H^T H)^{-1}, which is not built for a large PSF; use MYULA");
  if (!rc) rc = check_no_spectral(s->prob, "ULPDA", "its primal step through lmc_l2_prox's closed form is not wired into the primal-dual loop; use MYULA");
  if (!rc) rc = check_no_sense(s->prob, "ULPDA", "its primal step is the implicit step of f, which is diagonal in neither the pixel nor the Fourier basis for coil maps; use MYULA");
  if (!rc) rc = check_no_box(s->prob, "ULPDA", "its prior enters through the dual ball of g o A, which has no box form; use MYULA");
  if (rc) { delete s; return rc; }
  if (hipGetDevice(&s->device) != hipSuccess) { delete s; return fail(LMC_E_HIP, "hipGetDevice failed"); }
  s->kind = 1;
  s->C = cfg->n_chains;
  s->chain_offset = cfg->chain_offset;
  s->tau = cfg->tau; s->mu = cfg->mu; s->theta = cfg->theta;
  s->gfirst = cfg->gfirst != 0; s->cg_niter = cfg->cg_niter; s->warm = cfg->warm != 0;
  s->z = cfg->z_dev;
  s->seed = cfg->seed;
  s->noise_mode = cfg->noise_mode;
  s->moments = cfg->moments; s->burn_in = cfg->burn_in; s->thin = cfg->thin < 1 ? 1 : cfg->thin;
  s->base.key0 = (uint32_t)(s->seed & 0xFFFFFFFFu);
  s->base.key1 = (uint32_t)(s->seed >> 32);
  s->base.chain_offset = (uint32_t)s->chain_offset;
  const size_t n = (size_t)s->C * s->prob.H * s->prob.W, img = (size_t)s->prob.H * s->prob.W;
  hipError_t e = hipSuccess;
  auto alloc = [&](float** p, size_t count) { if (e == hipSuccess) e = s->own.alloc(p, count, true); };
  alloc(&s->x[0], n); alloc(&s->xhat, n); alloc(&s->ydual, 2 * n); alloc(&s->uw, n); alloc(&s->rhs, n);
  if (s->noise_mode == LMC_NOISE_PHILOX) alloc(&s->xi, n);
  if (s->prob.data_kind == LMC_DATA_BLUR) {
    alloc(&s->cr, n); alloc(&s->cp, n); alloc(&s->cq, n); alloc(&s->ctmp, n); alloc(&s->htb, img); alloc(&s->zero_y, img);
    if (lmc::cheb_pair_supported(s->prob.H, s->prob.W, s->prob.taps)) alloc(&s->uw2, n);
    if (e == hipSuccess) e = s->own.alloc(&s->scal, 4 * (size_t)s->C + 1, false);
    if (e == hipSuccess) e = lmc::launch_blur(s->prob.y, s->htb, 1, s->prob.H, s->prob.W, s->prob.taps, 1, nullptr);   // H^T b
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (s->prob.ncvx_kind != LMC_NCVX_NONE && !s->ctmp) alloc(&s->ctmp, n);      // pointwise data terms: the pre-step of L2_ncvx_tv.prox needs its own array
  if (e == hipSuccess) {     // the inner prox of the ME-TV term (the pre-step adds it with weight tau) and the energies
    lmc::StepArgs probe{};
    probe.t = s->tau;
    e = prepare(s->ws, s->prob, probe, s->C, 0.f, kForStep | kForEnergies, nullptr);
  }
  if (e == hipSuccess) e = alloc_moments(s);
  if (e != hipSuccess) return alloc_failed(s, e);
  s->kernel_name = "(no step launched yet)";
  *out = s;
  return LMC_OK;
}

int lmc_sampler_set_dual(lmc_sampler* s, const float* y_dev, void* stream) {
  if (!s || !y_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  if (s->kind != 1) return fail(LMC_E_STATE, "not a ULPDA sampler");
  HIP_TRY(hipMemcpyAsync(s->ydual, y_dev, sizeof(float) * 2 * (size_t)s->C * s->prob.H * s->prob.W, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_sampler_get_dual(lmc_sampler* s, float* y_dev, void* stream) {
  if (!s || !y_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  if (s->kind != 1) return fail(LMC_E_STATE, "not a ULPDA sampler");
  HIP_TRY(hipMemcpyAsync(y_dev, s->ydual, sizeof(float) * 2 * (size_t)s->C * s->prob.H * s->prob.W, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_sampler_set_steps(lmc_sampler* s, float tau, float mu) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  if (s->kind != 1) return fail(LMC_E_STATE, "not a ULPDA sampler");
  if (!(tau > 0.f) || !(mu > 0.f)) return fail(LMC_E_INVALID, "tau and mu must be > 0");
  s->tau = tau; s->mu = mu;
  return LMC_OK;
}

int64_t lmc_sampler_iteration(const lmc_sampler* s) { return s ? s->iteration : -1; }

int lmc_sampler_set_iteration(lmc_sampler* s, int64_t it) {
  if (!s || it < 0 || it > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  s->iteration = it;
  return LMC_OK;
}

int lmc_sampler_energies(lmc_sampler* s, double* f_out_dev, double* g_out_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return sampler_energies_at(s, s->x[s->cur], f_out_dev, g_out_dev, S(stream));
}

int lmc_sampler_noise(lmc_sampler* s, int64_t iteration, float* out_dev, void* stream) {
  if (!s || !out_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  if (iteration < 0 || iteration > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  HIP_TRY(lmc::launch_noise(out_dev, s->C, s->prob.H, s->prob.W, s->base.key0, s->base.key1, (uint32_t)iteration,
                            s->base.chain_offset, S(stream)));
  return LMC_OK;
}

int lmc_sampler_last_step_timing(lmc_sampler* s, float* total_ms, int32_t* n_launches) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->timed || s->last_launches < 1)
    return fail(LMC_E_STATE, "no timed lmc_sampler_step call to report (lmc_sampler_enable_timing first)");
  HIP_TRY(hipEventSynchronize(s->ev[2 * s->last_launches - 1]));
  float ms = 0.f;
  for (int k = 0; k < s->last_launches; ++k) {
    float d = 0.f;
    HIP_TRY(hipEventElapsedTime(&d, s->ev[2 * k], s->ev[2 * k + 1]));
    ms += d;
  }
  if (total_ms) *total_ms = ms;
  if (n_launches) *n_launches = s->last_launches;
  return LMC_OK;
}

const char* lmc_sampler_kernel_name(const lmc_sampler* s) { return s ? s->kernel_name.c_str() : ""; }

int lmc_sampler_tv_exit_stats(lmc_sampler* s, int32_t which, int32_t* passes_dev, uint64_t* reruns_host, void* stream) {
  if (!s || (which != 0 && which != 1)) return fail(LMC_E_INVALID, "bad arguments");
  DeviceGuard dg(s->device);
  RtState& rt = which == 0 ? s->ws.rt_tv : s->ws.rt_me;
  if (!rt.kc) return fail(LMC_E_STATE, "this sampler does not run the device-side early exit for that prox (tv_rtol / ncvx_rtol = 0, or the pass-by-pass path)");
  hipStream_t st = S(stream);
  if (passes_dev) HIP_TRY(hipMemcpyAsync(passes_dev, rt.pred, sizeof(int) * (size_t)s->C, hipMemcpyDeviceToDevice, st));
  unsigned long long r[4] = {0, 0, 0, 0};
  if (reruns_host) HIP_TRY(hipMemcpyAsync(r, rt.reruns, sizeof r, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (reruns_host) for (int i = 0; i < 4; ++i) reruns_host[i] = r[i];
  return LMC_OK;
}

}  // extern "C"
