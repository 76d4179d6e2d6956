// The multi-channel MYULA sampler under the vectorial TV prior (lmc_mch_*; include/lmc_atomi.h): a handle type of its own that composes existing parts.
// One iteration = lmc_vtv.hip's prox over all chains and channels into a buffer of the handle, then per channel one launch_step of the same problem
// without a prior, which takes that channel's block of the buffer as a ready-made prox (StepArgs::prox_ext, the route of LMC_PRIOR_WAVELET_L1).  The kept
// iterates go through one Accumulators per channel, the data energies through problem_energies per channel.
// State, injected noise and the prox buffer are [n_channels][n_chains][H][W]: channel-major, each channel's chains contiguous.
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "lmc_device.h"
#include "lmc_host.h"

using namespace lmc::host;

struct lmc_mch {
  int device = -1;
  int nch = 0, C = 0, H = 0, W = 0;
  int64_t chain_offset = 0;
  float tau = 0, gamma = 0, epsg = 1;
  uint64_t seed = 0;
  int noise_mode = 0;
  int moments = 0, burn_in = 0, thin = 1;
  int64_t iteration = 0;
  // the prior: sigma VTV, its prox by niter dual iterations, the box
  float sigma = 0.f, tv_step = 0.125f;
  int niter = 0;
  float betas[lmc::kMaxTvIters] = {};
  int box = 0;
  float box_lo = 0.f, box_hi = 0.f;
  Problem prob[LMC_MAX_CHANNELS];          // channel ch's problem: its plane of y and its mask, no prior
  lmc::StepArgs base[LMC_MAX_CHANNELS];    // its update, with the Philox key of the channel
  Accumulators acc[LMC_MAX_CHANNELS];
  Workspace ws;                            // the work buffers of a channel's step and energy launches (the channels run one after the other)
  Owned own;
  float* x[2] = {nullptr, nullptr};
  int cur = 0;
  float* prox = nullptr;                   // the prox of the current state
  float* vstate[2] = {nullptr, nullptr};   // chained prox: the dual state ping-pong
  double* vpart = nullptr;                 // the partial sums of the value
  double* fch = nullptr;                   // [n_channels][C]: f per channel and chain
  std::string kernel_name;

  size_t img() const { return (size_t)H * W; }
  size_t block() const { return (size_t)C * H * W; }      // one channel's chains
};

namespace {

// f[c] = sum_ch fch[ch][c], in channel order
__global__ void mch_sum_channels_kernel(const double* __restrict__ fch, int nch, int C, double* __restrict__ f) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a = 0.0;
  for (int ch = 0; ch < nch; ++ch) a += fch[(size_t)ch * C + c];
  f[c] = a;
}

void destroy(lmc_mch* s) {
  s->own.release();
  s->ws.release();
  for (Accumulators& a : s->acc) a.release();
  delete s;
}

int alloc_failed(lmc_mch* s, hipError_t e) {
  const int rc = fail(e == hipErrorOutOfMemory ? LMC_E_NOMEM : LMC_E_HIP, "sampler allocation failed: %s", hipGetErrorString(e));
  destroy(s);
  return rc;
}

bool kept(const lmc_mch* s, int64_t it) { return s->moments && it >= s->burn_in && (it - s->burn_in) % s->thin == 0; }

}  // namespace

extern "C" {

int lmc_mch_create(const lmc_mch_config* cfg, lmc_mch** out) {
  if (!cfg || !out) return fail(LMC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(lmc_mch_config))
    return fail(LMC_E_INVALID, "lmc_mch_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(lmc_mch_config));
  if (cfg->n_channels < 1 || cfg->n_channels > LMC_MAX_CHANNELS) return fail(LMC_E_INVALID, "n_channels %d outside 1..%d", cfg->n_channels, LMC_MAX_CHANNELS);
  if (cfg->n_chains < 1) return fail(LMC_E_INVALID, "n_chains must be >= 1");
  if (cfg->chain_offset < 0 || cfg->chain_offset + cfg->n_chains > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "global chain ids must fit 32 bits");
  if (!(cfg->tau > 0.f) || !(cfg->gamma > 0.f)) return fail(LMC_E_INVALID, "tau and gamma must be > 0");
  if (!(cfg->epsg >= 0.f)) return fail(LMC_E_INVALID, "epsg must be >= 0");
  if (cfg->noise_mode < LMC_NOISE_PHILOX || cfg->noise_mode > LMC_NOISE_NONE) return fail(LMC_E_INVALID, "bad noise_mode");
  if (cfg->moments && cfg->thin < 1) return fail(LMC_E_INVALID, "thin must be >= 1");
  if (cfg->moments && cfg->burn_in < 0) return fail(LMC_E_INVALID, "burn_in must be >= 0");
  lmc_problem p = cfg->problem;
  if (p.struct_size != sizeof(lmc_problem))
    return fail(LMC_E_INVALID, "lmc_problem.struct_size %u != %zu (ABI mismatch)", p.struct_size, sizeof(lmc_problem));
  if (p.prior_kind == LMC_PRIOR_TGV)
    return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: LMC_PRIOR_TGV acts on single-plane images (lmc_myula_create, lmc_skrock_create); a vectorial TGV is not built");
  if (p.prior_kind != LMC_PRIOR_VTV) return fail(LMC_E_INVALID, "lmc_mch_create: prior_kind must be LMC_PRIOR_VTV (got %d)", p.prior_kind);
  if (p.data_kind > LMC_DATA_MASK && p.data_kind <= LMC_DATA_SENSE)
    return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: data_kind %d is not built per channel: LMC_DATA_NONE, IDENTITY, BLUR or MASK", p.data_kind);
  if (p.ncvx_kind != LMC_NCVX_NONE) return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: the non-convex terms are not built for multi-channel images: ncvx_kind must be LMC_NCVX_NONE");
  if (p.tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: tv_rtol > 0 (early exit of the prox) is not built for LMC_PRIOR_VTV: use the fixed count, tv_rtol = 0");
  if (p.tv_warm) return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: tv_warm (warm-started dual) is not built for LMC_PRIOR_VTV");
  if (p.prox_scale) return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: prox_scale (array-valued epsg) is built for the closed-form priors only");
  if (p.tv_lagged_output) return fail(LMC_E_UNSUPPORTED, "lmc_mch_create: tv_lagged_output is not built for LMC_PRIOR_VTV: the prox returns the iterate after tv_niter dual updates");
  if (p.tv_niter < 1 || p.tv_niter > lmc::kMaxTvIters) return fail(LMC_E_INVALID, "tv_niter %d outside 1..%d", p.tv_niter, lmc::kMaxTvIters);
  if (p.H < 1 || p.W < 1 || (int64_t)p.H * p.W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad image size %dx%d", p.H, p.W);
  if (cfg->mask_channel_stride != 0 && cfg->mask_channel_stride != (int64_t)p.H * p.W)
    return fail(LMC_E_INVALID, "mask_channel_stride must be 0 (one mask for all channels) or H * W = %lld (one per channel), got %lld", (long long)p.H * p.W,
                (long long)cfg->mask_channel_stride);
  if ((int64_t)cfg->n_channels * cfg->n_chains > (1 << 24)) return fail(LMC_E_INVALID, "n_channels * n_chains above 2^24");
  // everything else of the problem is checked as for the isotropic TV prior, whose fields the kind reads
  p.prior_kind = LMC_PRIOR_TV_ISO;
  lmc_mch* s = new (std::nothrow) lmc_mch();
  if (!s) return fail(LMC_E_NOMEM, "host allocation failed");
  Problem& q0 = s->prob[0];
  int rc = load_problem(&p, q0);
  if (rc) { delete s; return rc; }
  if (hipGetDevice(&s->device) != hipSuccess) { delete s; return fail(LMC_E_HIP, "hipGetDevice failed"); }
  s->nch = cfg->n_channels; s->C = cfg->n_chains; s->H = q0.H; s->W = q0.W;
  s->chain_offset = cfg->chain_offset;
  s->tau = cfg->tau; s->gamma = cfg->gamma; s->epsg = cfg->epsg;
  s->seed = cfg->seed;
  s->noise_mode = cfg->noise_mode;
  s->moments = cfg->moments; s->burn_in = cfg->burn_in; s->thin = cfg->thin < 1 ? 1 : cfg->thin;
  s->sigma = q0.prior_sigma; s->tv_step = q0.tv_step; s->niter = q0.tv_niter;
  std::memcpy(s->betas, q0.betas, sizeof s->betas);
  s->box = q0.box; s->box_lo = q0.box_lo; s->box_hi = q0.box_hi;
  // channel ch: the same operator on its own plane of y (and of the mask), no prior and no box -- both live in the prox that the step consumes
  q0.prior_kind = LMC_PRIOR_NONE; q0.prior_sigma = 0.f; q0.tv_niter = 0; q0.tv_niter_asked = 0; q0.box = 0;
  for (int ch = s->nch - 1; ch >= 0; --ch) {
    Problem& q = s->prob[ch];
    q = q0;
    if (q.y) q.y = q0.y + (size_t)ch * s->img();
    if (q.mask) q.mask = q0.mask + (size_t)ch * cfg->mask_channel_stride;
    rc = check_step_problem(q, s->tau / s->gamma);
    if (!rc) rc = make_step_args(q, 1.f - s->tau / s->gamma, s->tau, s->tau / s->gamma, s->epsg * s->gamma, std::sqrt(2.f * s->tau), s->base[ch]);
    if (rc) { delete s; return rc; }
    lmc::StepArgs& A = s->base[ch];
    A.C = s->C;
    A.noise_mode = s->noise_mode;
    A.key0 = (uint32_t)(s->seed & 0xFFFFFFFFu);
    A.key1 = (uint32_t)(s->seed >> 32) + (uint32_t)ch;       // channel ch draws the field of the seed (seed + (ch << 32)) mod 2^64
    A.chain_offset = (uint32_t)s->chain_offset;
  }
  const size_t n = (size_t)s->nch * s->block();
  hipError_t e = s->own.alloc(&s->x[0], n, true);
  if (e == hipSuccess) e = s->own.alloc(&s->x[1], n, false);
  if (e == hipSuccess) e = s->own.alloc(&s->prox, n, false);
  const size_t ns = lmc::vtv_state_floats(s->C, s->nch, s->H, s->W, s->niter);
  for (int i = 0; i < 2 && e == hipSuccess && ns; ++i) e = s->own.alloc(&s->vstate[i], ns, false);
  if (e == hipSuccess) e = s->own.alloc(&s->vpart, lmc::vtv_value_partials(s->C, s->H, s->W), false);
  if (e == hipSuccess) e = s->own.alloc(&s->fch, (size_t)s->nch * s->C, false);
  // every work buffer of a channel's step and energy launches, here and never inside lmc_mch_step (the channels have the same needs)
  for (int ch = 0; ch < s->nch && e == hipSuccess; ++ch) {
    lmc::StepArgs probe = s->base[ch];
    probe.prox_ext = s->prox;
    e = prepare(s->ws, s->prob[ch], probe, s->C, s->epsg * s->gamma, kForStep | kForEnergyF, nullptr);
  }
  for (int ch = 0; ch < s->nch && e == hipSuccess && s->moments; ++ch) e = s->acc[ch].alloc(s->C, s->chain_offset, s->H, s->W);
  if (e != hipSuccess) return alloc_failed(s, e);
  s->kernel_name = "(no step launched yet)";
  *out = s;
  return LMC_OK;
}

void lmc_mch_destroy(lmc_mch* s) {
  if (!s) return;
  DeviceGuard dg(s->device);
  destroy(s);
}

int lmc_mch_set_state(lmc_mch* s, const float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  HIP_TRY(hipMemcpyAsync(s->x[s->cur], x_dev, sizeof(float) * s->nch * s->block(), hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_mch_get_state(lmc_mch* s, float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  HIP_TRY(hipMemcpyAsync(x_dev, s->x[s->cur], sizeof(float) * s->nch * s->block(), hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_mch_step(lmc_mch* s, int32_t n_iters, const float* noise_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (n_iters < 0) return fail(LMC_E_INVALID, "n_iters < 0");
  if (s->noise_mode == LMC_NOISE_INJECTED && !noise_dev && n_iters > 0) return fail(LMC_E_INVALID, "noise_mode is INJECTED but noise_dev is NULL");
  if (s->noise_mode != LMC_NOISE_INJECTED && noise_dev) return fail(LMC_E_INVALID, "noise_dev given but noise_mode is not INJECTED");
  if (s->iteration + n_iters > 0xFFFFFFFFLL) return fail(LMC_E_STATE, "iteration counter would exceed 32 bits");
  hipStream_t st = S(stream);
  const size_t blk = s->block(), per_iter = s->nch * blk;
  const float pt = s->epsg * s->gamma * s->sigma;       // the prox parameter t sigma
  for (int k = 0; k < n_iters; ++k) {
    const float* xin = s->x[s->cur];
    float* xout = s->x[s->cur ^ 1];
    const float* px = xin;                               // t sigma = 0: the prox is the identity
    std::string name;
    if (pt > 0.f) {
      HIP_TRY(lmc::launch_vtv_prox(xin, s->prox, s->C, s->nch, (int64_t)blk, s->H, s->W, pt, s->tv_step, s->betas, s->niter, s->box, s->box_lo, s->box_hi,
                                   s->vstate[0], s->vstate[1], st));
      px = s->prox;
      name = s->box ? "vtv_prox_kernel(box) + " : "vtv_prox_kernel + ";
    }
    const char* kname = nullptr;
    for (int ch = 0; ch < s->nch; ++ch) {
      lmc::StepArgs A = s->base[ch];
      A.x_in = xin + ch * blk;
      A.x_out = xout + ch * blk;
      A.prox_ext = px + ch * blk;
      A.iteration = (uint32_t)s->iteration;
      A.noise = noise_dev ? noise_dev + (size_t)k * per_iter + ch * blk : nullptr;
      sanitize_pointers(A);
      hipError_t e = launch_step(A, s->prob[ch], s->ws, st, &kname);
      if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "no step-kernel variant covers this configuration");
      HIP_TRY(e);
    }
    if (kname) s->kernel_name = name + kname;
    s->cur ^= 1;
    if (kept(s, s->iteration)) {
      for (int ch = 0; ch < s->nch; ++ch) {
        HIP_TRY(s->acc[ch].reduce(s->x[s->cur] + ch * blk, st));
        s->acc[ch].count += (uint64_t)s->C;
      }
    }
    ++s->iteration;
  }
  return LMC_OK;
}

int64_t lmc_mch_iteration(const lmc_mch* s) { return s ? s->iteration : -1; }

int lmc_mch_set_iteration(lmc_mch* s, int64_t it) {
  if (!s || it < 0 || it > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  s->iteration = it;
  return LMC_OK;
}

int lmc_mch_get_moments(lmc_mch* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  const size_t mb = sizeof(double) * s->img();
  for (int ch = 0; ch < s->nch; ++ch) {
    if (sum_dev) HIP_TRY(hipMemcpyAsync(sum_dev + ch * s->img(), s->acc[ch].s1, mb, hipMemcpyDeviceToDevice, S(stream)));
    if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev + ch * s->img(), s->acc[ch].s2, mb, hipMemcpyDeviceToDevice, S(stream)));
  }
  HIP_TRY(hipStreamSynchronize(S(stream)));
  if (count) *count = s->acc[0].count;
  return LMC_OK;
}

int lmc_mch_reset_moments(lmc_mch* s, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  for (int ch = 0; ch < s->nch; ++ch) {
    const int rc = s->acc[ch].reset(S(stream));
    if (rc) return rc;
  }
  return LMC_OK;
}

int lmc_mch_energies(lmc_mch* s, double* f_out_dev, double* g_out_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  hipStream_t st = S(stream);
  const float* x = s->x[s->cur];
  if (f_out_dev) {
    for (int ch = 0; ch < s->nch; ++ch) {
      const int rc = problem_energies(s->prob[ch], x + ch * s->block(), s->C, s->fch + (size_t)ch * s->C, nullptr, s->ws, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(mch_sum_channels_kernel, dim3((unsigned)((s->C + 255) / 256)), dim3(256), 0, st, s->fch, s->nch, s->C, f_out_dev);
    HIP_TRY(hipGetLastError());
  }
  if (g_out_dev)
    HIP_TRY(lmc::launch_vtv_value(x, s->C, s->nch, (int64_t)s->block(), s->H, s->W, (double)s->sigma, s->vpart, g_out_dev, st));
  return LMC_OK;
}

int lmc_mch_noise(lmc_mch* s, int64_t iteration, float* out_dev, void* stream) {
  if (!s || !out_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  if (iteration < 0 || iteration > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  for (int ch = 0; ch < s->nch; ++ch)
    HIP_TRY(lmc::launch_noise(out_dev + ch * s->block(), s->C, s->H, s->W, s->base[ch].key0, s->base[ch].key1, (uint32_t)iteration, s->base[ch].chain_offset,
                              S(stream)));
  return LMC_OK;
}

const char* lmc_mch_kernel_name(const lmc_mch* s) { return s ? s->kernel_name.c_str() : ""; }

}  // extern "C"
