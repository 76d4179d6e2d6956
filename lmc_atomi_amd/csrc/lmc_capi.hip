// extern "C" boundary of liblmc_atomi.so (see include/lmc_atomi.h): the stateless entry points.  Argument checks happen
// HERE, on the host, before any kernel sees a pointer or a shape.  The samplers are in lmc_sampler.hip, RCCL in lmc_rccl.hip.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "lmc_host.h"

namespace lmc::host {
namespace {

thread_local std::string g_err;

constexpr int kMaxDevices = 64;
Workspace g_scratch_dev[kMaxDevices];     // grown on demand and never freed

// the argument checks the stateless transform calls share
int check_fft_call(const void* x_dev, const void* out_dev, int64_t n_img, int32_t H, int32_t W) {
  if (!x_dev || !out_dev || x_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (!lmc::fft_shape_ok(H, W)) return fail(LMC_E_UNSUPPORTED, "H and W must be powers of two in %d .. %d (got %dx%d)", lmc::kFftMin, lmc::kFftMax, H, W);
  return LMC_OK;
}

}  // namespace

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

Workspace& scratch_here() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return g_scratch_dev[(dev >= 0 && dev < kMaxDevices) ? dev : 0];
}

}  // namespace lmc::host

using namespace lmc::host;

extern "C" {

int lmc_version(void) { return LMC_ATOMI_ABI_VERSION; }

const char* lmc_last_error(void) { return g_err.c_str(); }

int lmc_device_info(int* device, int* n_cu, size_t* lds_bytes, size_t* hbm_bytes) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t pr;
  HIP_TRY(hipGetDeviceProperties(&pr, dev));
  if (device) *device = dev;
  if (n_cu) *n_cu = pr.multiProcessorCount;
  if (lds_bytes) *lds_bytes = pr.maxSharedMemoryPerMultiProcessor;
  if (hbm_bytes) *hbm_bytes = pr.totalGlobalMem;
  return LMC_OK;
}

int lmc_hbm_copy_probe(size_t bytes, int32_t reps, float* gbs_out, void* stream) {
  if (!gbs_out || reps < 1 || bytes < (1u << 20)) return fail(LMC_E_INVALID, "bad arguments (at least 1 MiB, reps >= 1)");
  const size_t n = (bytes / 16) * 4;                       // floats, a multiple of 4
  hipStream_t st = S(stream);
  float *x = nullptr, *y = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipMalloc(&x, n * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&y, n * sizeof(float));
  if (e == hipSuccess) e = hipMemsetAsync(x, 0, n * sizeof(float), st);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  float best = 0.f;
  for (int shape = 0; shape < lmc::hbm_copy_probe_shapes(); ++shape)     // launch shapes: what a plain copy reaches depends on them
    for (int r = 0; r < reps + 1 && e == hipSuccess; ++r) {   // the first pass warms up (page mapping, clocks)
      e = hipEventRecord(e0, st);
      if (e == hipSuccess) e = lmc::launch_hbm_copy_probe(x, y, n, shape, st);
      if (e == hipSuccess) e = hipEventRecord(e1, st);
      if (e == hipSuccess) e = hipEventSynchronize(e1);
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (e == hipSuccess && r > 0 && ms > 0.f) best = fmaxf(best, (float)(2.0 * (double)n * sizeof(float) / ((double)ms * 1e-3) / 1e9));
    }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (x) (void)hipFree(x);
  if (y) (void)hipFree(y);
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? LMC_E_NOMEM : LMC_E_HIP, "HBM probe failed: %s", hipGetErrorString(e));
  *gbs_out = best;
  return LMC_OK;
}

int lmc_blur(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* h_host, int32_t kh,
             int32_t kw, int32_t oy, int32_t ox, int32_t adjoint, void* stream) {
  if (!x_dev || !out_dev) return fail(LMC_E_INVALID, "NULL image pointer");
  if (x_dev == out_dev) return fail(LMC_E_INVALID, "lmc_blur cannot run in place");
  if (n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  lmc::BlurTaps T;
  int rc = fill_taps(T, h_host, kh, kw, oy, ox);
  if (rc) return rc;
  HIP_TRY(lmc::launch_blur(x_dev, out_dev, n_img, H, W, T, adjoint != 0, S(stream)));
  return LMC_OK;
}

int lmc_psf_separable(const float* h_host, int32_t kh, int32_t kw, float* u_out, float* v_out) {
  if (!h_host) return fail(LMC_E_INVALID, "PSF pointer is NULL");
  if (kh < 1 || kw < 1 || kh > lmc::kPsfMax || kw > lmc::kPsfMax) return fail(LMC_E_INVALID, "PSF %dx%d outside 1..%d", kh, kw, lmc::kPsfMax);
  return lmc::psf_separable(h_host, kh, kw, u_out, v_out);
}

int lmc_psf_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* h_host, int32_t kh, int32_t kw, int32_t oy,
                  int32_t ox, int32_t adjoint, int32_t separable, void* stream) {
  if (!x_dev || !out_dev) return fail(LMC_E_INVALID, "NULL image pointer");
  if (x_dev == out_dev) return fail(LMC_E_INVALID, "lmc_psf_apply cannot run in place");
  if (n_img < 1 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (!h_host) return fail(LMC_E_INVALID, "PSF pointer is NULL");
  if (kh < 1 || kw < 1 || kh > lmc::kPsfMax || kw > lmc::kPsfMax) return fail(LMC_E_INVALID, "PSF %dx%d outside 1..%d", kh, kw, lmc::kPsfMax);
  if (oy < 0 || oy >= kh || ox < 0 || ox >= kw) return fail(LMC_E_INVALID, "PSF offset (%d,%d) outside the kernel", oy, ox);
  if (separable < 0 || separable > 2) return fail(LMC_E_INVALID, "separable must be 0 (auto), 1 (require) or 2 (forbid)");
  lmc::PsfOp P;
  if (!lmc::psf_prepare(P, h_host, kh, kw, oy, ox, separable))
    return fail(LMC_E_INVALID, "separable = 1 on a kernel that is no outer product to 2^-22 of every tap (lmc_psf_separable)");
  HIP_TRY(scratch_here().bind_psf(P, 0, S(stream)));
  HIP_TRY(lmc::launch_psf(P, adjoint != 0, lmc::kPsfRaw, x_dev, out_dev, nullptr, nullptr, n_img, H, W, 0.f, 0.f, S(stream)));
  return LMC_OK;
}

int lmc_rfft2(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream) {
  int rc = check_fft_call(x_dev, out_dev, n_img, H, W);
  if (rc) return rc;
  lmc::FftOp F;
  HIP_TRY(scratch_here().bind_fft(F, 0, 0));
  float2* spec = reinterpret_cast<float2*>(out_dev);
  HIP_TRY(lmc::launch_fft_rows_fwd(x_dev, spec, F.tw, n_img, H, W, S(stream)));
  HIP_TRY(lmc::launch_fft_cols(lmc::kFftColFwd, spec, nullptr, F.tw, n_img, H, W, 0.f, S(stream)));
  return LMC_OK;
}

int lmc_irfft2(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream) {
  int rc = check_fft_call(x_dev, out_dev, n_img, H, W);
  if (rc) return rc;
  lmc::FftOp F;
  const size_t nf = lmc::fft_spec_floats(n_img, H, W);
  HIP_TRY(scratch_here().bind_fft(F, nf, 0));
  HIP_TRY(hipMemcpyAsync(F.spec, x_dev, sizeof(float) * nf, hipMemcpyDeviceToDevice, S(stream)));      // the column pass runs in place: on a copy
  HIP_TRY(lmc::launch_fft_cols(lmc::kFftColInv, F.spec, nullptr, F.tw, n_img, H, W, 0.f, S(stream)));
  HIP_TRY(lmc::launch_fft_rows_inv(lmc::kFftStore, F.spec, out_dev, nullptr, F.tw, n_img, H, W, 0.f, 0.f, S(stream)));
  return LMC_OK;
}

int lmc_spectral_filter(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* m_dev, void* stream) {
  int rc = check_fft_call(x_dev, out_dev, n_img, H, W);
  if (rc) return rc;
  if (!m_dev) return fail(LMC_E_INVALID, "the multiplier m_dev is NULL");
  lmc::FftOp F;
  HIP_TRY(scratch_here().bind_fft(F, lmc::fft_spec_floats(n_img, H, W), 0));
  HIP_TRY(lmc::launch_fft_rows_fwd(x_dev, F.spec, F.tw, n_img, H, W, S(stream)));
  HIP_TRY(lmc::launch_fft_cols(lmc::kFftMul, F.spec, m_dev, F.tw, n_img, H, W, 0.f, S(stream)));
  HIP_TRY(lmc::launch_fft_rows_inv(lmc::kFftStore, F.spec, out_dev, nullptr, F.tw, n_img, H, W, 0.f, 0.f, S(stream)));
  return LMC_OK;
}

int lmc_spectral_tables(const double* G_host, const double* b_host, int32_t H, int32_t W, float* out_host) {
  if (!G_host || !b_host || !out_host) return fail(LMC_E_INVALID, "NULL pointer");
  if (H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape H=%d W=%d", H, W);
  if (!lmc::fft_shape_ok(H, W)) return fail(LMC_E_UNSUPPORTED, "H and W must be powers of two in %d .. %d (got %dx%d)", lmc::kFftMin, lmc::kFftMax, H, W);
  lmc::fft_tables(G_host, b_host, H, W, out_host);
  return LMC_OK;
}

int lmc_sense_apply(const float* desc_dev, const float* in_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t n_coils, int32_t adjoint,
                    void* stream) {
  if (!desc_dev) return fail(LMC_E_INVALID, "the descriptor desc_dev is NULL");
  if (!in_dev || !out_dev) return fail(LMC_E_INVALID, "NULL image pointer");
  if (in_dev == out_dev) return fail(LMC_E_INVALID, "lmc_sense_apply cannot run in place");
  if (n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (n_coils < 1 || n_coils > lmc::kSenseMaxCoils) return fail(LMC_E_INVALID, "n_coils %d outside 1..%d", n_coils, lmc::kSenseMaxCoils);
  if (!lmc::fft_shape_ok(H, W)) return fail(LMC_E_UNSUPPORTED, "H and W must be powers of two in %d .. %d (got %dx%d)", lmc::kFftMin, lmc::kFftMax, H, W);
  lmc::SenseOp Sn;
  Sn.on = 1; Sn.n_coils = n_coils; Sn.desc = desc_dev;
  HIP_TRY(scratch_here().bind_sense(Sn, adjoint ? lmc::sense_spec_floats(n_img, H, W) : 0, 0, 0));
  HIP_TRY(lmc::launch_sense_apply(Sn, in_dev, out_dev, n_img, H, W, adjoint != 0, S(stream)));
  return LMC_OK;
}

double lmc_sense_lipschitz(const float* desc_host, int32_t H, int32_t W, int32_t n_coils) {
  if (!desc_host) return (double)fail(LMC_E_INVALID, "the descriptor desc_host is NULL");
  if (H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return (double)fail(LMC_E_INVALID, "bad shape H=%d W=%d", H, W);
  if (n_coils < 1 || n_coils > lmc::kSenseMaxCoils) return (double)fail(LMC_E_INVALID, "n_coils %d outside 1..%d", n_coils, lmc::kSenseMaxCoils);
  return lmc::sense_lipschitz(desc_host, H, W, n_coils);
}

// the argument checks the two Radon calls share; R: the validated operator
static int check_radon_call(const float* angles_host, int32_t n_angles, int32_t n_det, int32_t H, int32_t W, lmc::RadonOp& R) {
  if (H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad image size %dx%d", H, W);
  if (!angles_host) return fail(LMC_E_INVALID, "angles pointer is NULL");
  if (n_angles < 1 || n_angles > lmc::kRadonMaxAngles) return fail(LMC_E_INVALID, "n_angles %d outside 1..%d", n_angles, lmc::kRadonMaxAngles);
  if (n_det < 1 || n_det > lmc::kRadonMaxDet) return fail(LMC_E_INVALID, "n_det %d outside 1..%d", n_det, lmc::kRadonMaxDet);
  for (int a = 0; a < n_angles; ++a)
    if (!std::isfinite(angles_host[a])) return fail(LMC_E_INVALID, "angle %d is not finite", a);
  if (H > lmc::kRadonMaxSide || W > lmc::kRadonMaxSide) return fail(LMC_E_UNSUPPORTED, "Radon operator: image sides up to %d (got %dx%d)", lmc::kRadonMaxSide, H, W);
  lmc::radon_prepare(R, angles_host, n_angles, n_det);
  return LMC_OK;
}

int lmc_radon_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* angles_host, int32_t n_angles, int32_t n_det,
                    int32_t adjoint, void* stream) {
  if (!x_dev || !out_dev) return fail(LMC_E_INVALID, "NULL image pointer");
  if (x_dev == out_dev) return fail(LMC_E_INVALID, "lmc_radon_apply cannot run in place");
  if (n_img < 1) return fail(LMC_E_INVALID, "bad n_img %lld", (long long)n_img);
  lmc::RadonOp R;
  int rc = check_radon_call(angles_host, n_angles, n_det, H, W, R);
  if (rc) return rc;
  HIP_TRY(scratch_here().bind_radon(R, H, W, 0, S(stream)));
  if (adjoint) HIP_TRY(lmc::launch_radon_adjoint(R, lmc::kRadonRaw, x_dev, out_dev, nullptr, n_img, H, W, 0.f, 0.f, S(stream)));
  else HIP_TRY(lmc::launch_radon_forward(R, lmc::kRadonRaw, x_dev, out_dev, nullptr, n_img, H, W, S(stream)));
  return LMC_OK;
}

int lmc_radon_tables(const float* angles_host, int32_t n_angles, int32_t n_det, int32_t H, int32_t W, float* ax_out, float* by_out) {
  lmc::RadonOp R;
  int rc = check_radon_call(angles_host, n_angles, n_det, H, W, R);
  if (rc) return rc;
  std::vector<float> tab(lmc::radon_table_floats(n_angles, H, W));
  lmc::radon_tables(R, H, W, tab.data());
  if (ax_out) std::memcpy(ax_out, tab.data(), sizeof(float) * (size_t)n_angles * W);
  if (by_out) std::memcpy(by_out, tab.data() + (size_t)n_angles * W, sizeof(float) * (size_t)n_angles * H);
  return LMC_OK;
}

int lmc_gradient(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream) {
  if (!x_dev || !out_dev || x_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers");
  if (n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape");
  HIP_TRY(lmc::launch_gradient(x_dev, out_dev, n_img, H, W, false, S(stream)));
  return LMC_OK;
}

int lmc_gradient_adjoint(const float* y_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream) {
  if (!y_dev || !out_dev || y_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers");
  if (n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad shape");
  HIP_TRY(lmc::launch_gradient(y_dev, out_dev, n_img, H, W, true, S(stream)));
  return LMC_OK;
}

int lmc_fused_eval(const lmc_problem* prob, const float* x_dev, float* out_dev, int64_t n_img, float a, float t, float b,
                   float pt, void* stream) {
  Problem q;
  int rc = load_problem(prob, q);
  if (rc) return rc;
  if (!x_dev || !out_dev || x_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || n_img > (1 << 24)) return fail(LMC_E_INVALID, "bad n_img %lld", (long long)n_img);
  if (q.prox_scale) return fail(LMC_E_UNSUPPORTED, "prox_scale (array-valued epsg) belongs to the MYULA sampler");
  rc = check_step_problem(q, b);
  if (rc) return rc;
  lmc::StepArgs A;
  rc = make_step_args(q, a, t, b, pt, 0.f, A);
  if (rc) return rc;
  A.C = (int)n_img;
  A.x_in = x_dev;
  A.x_out = out_dev;
  sanitize_pointers(A);
  Workspace& sc = scratch_here();
  HIP_TRY(prepare(sc, q, A, n_img, pt, kForStep, S(stream)));
  if (t != 0.f && q.ncvx_kind == LMC_NCVX_ME_TV) {
    rc = me_tv_prox(q, x_dev, n_img, sc, S(stream));
    if (rc) return rc;
    A.extra = sc.extra.p;
    A.extra_coef = -q.ncvx_lambda / q.ncvx_gamma;
  }
  if (sc.tv_exit == 0 || sc.tv_exit == 1) {     // the early exit decided on the device
    rc = tv_prior_rt(q, pt, A, sc, S(stream));
    if (rc < 0) return rc;
    if (rc == 1) return LMC_OK;
    if (rc == 2) return fail(LMC_E_UNSUPPORTED, "early exit of the TV prox: no path covers this configuration");
  } else if (sc.tv_exit == 2) {     // the early-exit prox first, then the fused update with it as a ready-made prox
    rc = tv_prox_rtol(q, pt, x_dev, sc.prox.p, n_img, sc, S(stream));
    if (rc) return rc;
    A.prior_kind = LMC_PRIOR_NONE;
    A.prox_ext = sc.prox.p;
  }
  hipError_t e = launch_step(A, q, sc, S(stream), nullptr);
  if (e == hipErrorInvalidConfiguration)
    return fail(LMC_E_UNSUPPORTED, A.box ? "step_variant %d has no box-constrained form of this prior (TV: auto, 1 tile, 7 / 8 pipe where the pipe covers the problem)"
                                         : "no step-kernel variant covers this configuration", variant_of(q));
  HIP_TRY(e);
  return LMC_OK;
}

int lmc_energies(const lmc_problem* prob, const float* x_dev, int64_t n_img, double* f_out_dev, double* g_out_dev,
                 void* stream) {
  Problem q;
  int rc = load_problem(prob, q);
  if (rc) return rc;
  if (!x_dev || n_img < 1) return fail(LMC_E_INVALID, "bad arguments");
  rc = check_convex_terms(q);
  if (rc) return rc;
  Workspace& sc = scratch_here();
  HIP_TRY(prepare(sc, q, lmc::StepArgs{}, n_img, 0.f, (f_out_dev ? kForEnergyF : 0) | (g_out_dev ? kForEnergyG : 0), S(stream)));
  return problem_energies(q, x_dev, n_img, f_out_dev, g_out_dev, sc, S(stream));
}

size_t lmc_l2_prox_workspace_bytes(int64_t n_img, int32_t H, int32_t W) {
  const size_t n = (size_t)n_img * H * W;
  return ((5 * n * sizeof(float) + 7) / 8) * 8 + (4 * (size_t)n_img + 1) * sizeof(double);
}

int lmc_l2_prox(const lmc_problem* prob, const float* x_dev, float* out_dev, int64_t n_img, float tau, int32_t niter,
                int32_t warm, void* workspace_dev, void* stream) {
  Problem q;
  int rc = load_problem(prob, q);
  if (rc) return rc;
  rc = check_no_radon(q, "lmc_l2_prox", "the implicit step (I + tau sigma_f A^T A)^{-1} is not built for it");
  if (!rc) rc = check_no_term(q, lmc::kTermPois, "lmc_l2_prox", "its implicit step (I + tau grad f)^{-1} has no closed form");
  if (!rc) rc = check_no_term(q, lmc::kTermHub, "lmc_l2_prox", "the implicit step of the Huber loss under an operator is not built");
  if (!rc) rc = check_no_term(q, lmc::kTermWl2, "lmc_l2_prox", "the implicit step (I + tau sigma_f Op^T W Op)^{-1} is not built");
  if (!rc) rc = check_no_psf(q, "lmc_l2_prox", "the implicit step (I + tau sigma_f H^T H)^{-1} is not built for it");
  if (!rc) rc = check_no_sense(q, "lmc_l2_prox", "the implicit step (I + tau sigma_f A^H A)^{-1} is diagonal in neither the pixel nor the Fourier basis");
  if (rc) return rc;
  if (!x_dev || !out_dev || x_dev == out_dev || n_img < 1) return fail(LMC_E_INVALID, "bad arguments (in-place not allowed)");
  if (!(tau > 0.f)) return fail(LMC_E_INVALID, "tau must be > 0");
  hipStream_t st = S(stream);
  const float ts = tau * q.sigma_f;
  const size_t n = (size_t)n_img * q.H * q.W;
  Workspace& sc = scratch_here();
  if (q.fft.on) {      // the spectral data term: the implicit step in closed form, (vh + ts B) / (1 + ts A) between the two column transforms
    if (q.ncvx_kind != LMC_NCVX_NONE) return fail(LMC_E_UNSUPPORTED, "the spectral data term has no non-convex form: ncvx_kind must be LMC_NCVX_NONE");
    HIP_TRY(sc.bind_fft(q.fft, lmc::fft_spec_floats(n_img, q.H, q.W), 0));
    HIP_TRY(lmc::launch_fft_rows_fwd(x_dev, q.fft.spec, q.fft.tw, n_img, q.H, q.W, st));
    HIP_TRY(lmc::launch_fft_cols(lmc::kFftProx, q.fft.spec, q.fft.tab, q.fft.tw, n_img, q.H, q.W, ts, st));
    HIP_TRY(lmc::launch_fft_rows_inv(lmc::kFftStore, q.fft.spec, out_dev, nullptr, q.fft.tw, n_img, q.H, q.W, 0.f, 0.f, st));
    return LMC_OK;
  }
  if (q.ncvx_kind == LMC_NCVX_ME_TV && q.data_kind != LMC_DATA_NONE) {     // the inner prox of the ME-TV term: the buffers of a step that carries the term
    lmc::StepArgs probe{};
    probe.t = tau;
    HIP_TRY(prepare(sc, q, probe, n_img, 0.f, kForStep, st));
  }
  if (q.data_kind != LMC_DATA_BLUR) {
    const float* xin = x_dev;
    if (q.ncvx_kind != LMC_NCVX_NONE && q.data_kind != LMC_DATA_NONE) {
      // L2_ncvx_tv.prox with a pointwise data term: the pre-step of algs.py:213-223 first (x + tau lambda A^T(Ax / max(|Ax|, gamma)), or
      // x + tau lambda / gamma (x - prox_{gamma TV}(x))), then the closed-form solve.  (Round 3's matrix test found this path applying the solve to x itself.)
      HIP_TRY(sc.prox.need(n));
      if (q.ncvx_kind == LMC_NCVX_MC_TV) {
        HIP_TRY(lmc::ulpda_ncvx_rhs(x_dev, q.y, sc.prox.p, n_img, q.H, q.W, tau * q.ncvx_lambda, q.ncvx_gamma, 0.f, st));     // ts = 0: the H^T b slot adds nothing
      } else {
        rc = me_tv_prox(q, x_dev, n_img, sc, st);
        if (rc) return rc;
        HIP_TRY(lmc::ulpda_me_rhs(x_dev, sc.extra.p, q.y, sc.prox.p, n_img, q.H, q.W, tau * q.ncvx_lambda / q.ncvx_gamma, 0.f, st));
      }
      xin = sc.prox.p;
    }
    HIP_TRY(lmc::ulpda_pointwise_prox(xin, out_dev, q.y, q.mask, n_img, q.H, q.W, ts, q.data_kind, st));
    return LMC_OK;
  }
  if (niter < 1) return fail(LMC_E_INVALID, "niter must be >= 1");
  if (!workspace_dev) return fail(LMC_E_INVALID, "workspace_dev is NULL (see lmc_l2_prox_workspace_bytes)");
  float* w = static_cast<float*>(workspace_dev);
  float *rhs = w, *r = w + n, *p = w + 2 * n, *qq = w + 3 * n, *tmp = w + 4 * n;
  double* scal = reinterpret_cast<double*>(static_cast<char*>(workspace_dev) + ((5 * n * sizeof(float) + 7) / 8) * 8);
  // rhs = x + ts * H^T y  : H^T y into tmp (one image), then broadcast-add through the rhs kernel with y == 0
  HIP_TRY(lmc::launch_blur(q.y, tmp, 1, q.H, q.W, q.taps, 1, st));
  // ulpda_rhs computes x - tau*(A^T ydual) + ts*htb; with a zero dual field it is x + ts*htb.  The dual field needs 2n
  // floats: use r and p (both overwritten later by the solver) as a zeroed [n_img][2][H][W] field.
  if (q.ncvx_kind == LMC_NCVX_MC_TV) {
    HIP_TRY(lmc::ulpda_ncvx_rhs(x_dev, tmp, rhs, n_img, q.H, q.W, tau * q.ncvx_lambda, q.ncvx_gamma, ts, st));
  } else if (q.ncvx_kind == LMC_NCVX_ME_TV) {
    rc = me_tv_prox(q, x_dev, n_img, sc, st);
    if (rc) return rc;
    HIP_TRY(lmc::ulpda_me_rhs(x_dev, sc.extra.p, tmp, rhs, n_img, q.H, q.W, tau * q.ncvx_lambda / q.ncvx_gamma, ts, st));
  } else {
    HIP_TRY(hipMemsetAsync(r, 0, sizeof(float) * 2 * n, st));
    HIP_TRY(lmc::ulpda_rhs(x_dev, r, nullptr, tmp, rhs, n_img, q.H, q.W, 0.f, ts, st));
  }
  if (!warm) HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(float) * n, st));
  HIP_TRY(hipMemsetAsync(tmp, 0, sizeof(float) * (size_t)q.H * q.W, st));   // tmp (H^T y) is consumed: reuse its first image as the zero observation
  rc = cg_solve_fused(q, ts, out_dev, rhs, r, p, qq, scal, n_img, niter, tmp, st);
  if (rc) return rc;
  return LMC_OK;
}

int lmc_sgs_xstep(const lmc_problem* prob, const float* z_dev, const float* noise_dev, float* out_dev, int64_t n_img, float rho, void* stream) {
  return sgs_xstep(prob, z_dev, noise_dev, out_dev, n_img, rho, scratch_here(), S(stream));
}

int lmc_haar_l1_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, float thr, void* stream) {
  if (!x_dev || !out_dev || n_img < 1 || H < 8 || W < 8) return fail(LMC_E_INVALID, "bad arguments");
  if ((H & 7) || (W & 7)) return fail(LMC_E_UNSUPPORTED, "H and W must be multiples of 8 (got %dx%d)", H, W);
  if (!(thr >= 0.f)) return fail(LMC_E_INVALID, "threshold must be >= 0");
  HIP_TRY(lmc::launch_haar_prox(x_dev, out_dev, n_img, H, W, thr, S(stream)));
  return LMC_OK;
}

int lmc_wavelet_filter(int32_t p, double* h_out, int32_t* len_out) {
  if (!h_out) return fail(LMC_E_INVALID, "h_out is NULL");
  const int n = lmc::wavelet_filter(p, h_out);
  if (!n) return fail(LMC_E_INVALID, "p must be 1..%d (got %d)", lmc::kWaveletMaxP, p);
  if (len_out) *len_out = n;
  return LMC_OK;
}

// the argument checks the two stateless wavelet calls share
static int check_wavelet_call(const float* x_dev, const float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t p, int32_t levels) {
  if (!x_dev || !out_dev || x_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (!lmc::wavelet_shape_ok(H, W, p, levels))
    return fail(LMC_E_INVALID, "a %dx%d image does not take %d levels of db%d: p in 1..%d, levels in 1..%d, H and W multiples of 2^levels, "
                "min(H, W) >> (levels - 1) >= 2p", H, W, levels, p, lmc::kWaveletMaxP, LMC_MAX_WAVELET_LEVELS);
  return LMC_OK;
}

int lmc_wavelet_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t p, int32_t levels, int32_t inverse, void* stream) {
  int rc = check_wavelet_call(x_dev, out_dev, n_img, H, W, p, levels);
  if (rc) return rc;
  Workspace& sc = scratch_here();
  HIP_TRY(sc.wav.need(lmc::wavelet_ws_floats(n_img, H, W)));
  HIP_TRY(lmc::launch_wavelet_apply(x_dev, out_dev, n_img, H, W, p, levels, inverse != 0, sc.wav.p, S(stream)));
  return LMC_OK;
}

int lmc_wavelet_l1_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t p, int32_t levels, float thr, void* stream) {
  int rc = check_wavelet_call(x_dev, out_dev, n_img, H, W, p, levels);
  if (rc) return rc;
  if (!(thr >= 0.f)) return fail(LMC_E_INVALID, "threshold must be >= 0");
  Workspace& sc = scratch_here();
  HIP_TRY(sc.wav.need(lmc::wavelet_ws_floats(n_img, H, W)));
  HIP_TRY(lmc::launch_wavelet_prox(x_dev, out_dev, n_img, H, W, p, levels, thr, sc.wav.p, S(stream)));
  return LMC_OK;
}

// the argument checks the two stateless vectorial-TV calls share
static int check_vtv_call(const void* x_dev, const void* out_dev, int64_t n_img, int32_t n_channels, int64_t channel_stride, int32_t H, int32_t W) {
  if (!x_dev || !out_dev || x_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || n_img > (1 << 24) || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30)
    return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (n_channels < 1 || n_channels > LMC_MAX_CHANNELS) return fail(LMC_E_INVALID, "n_channels %d outside 1..%d", n_channels, LMC_MAX_CHANNELS);
  if (n_channels > 1 && channel_stride < n_img * (int64_t)H * W)
    return fail(LMC_E_INVALID, "channel_stride %lld is below n_img * H * W = %lld: the channels would overlap", (long long)channel_stride, (long long)(n_img * (int64_t)H * W));
  return LMC_OK;
}

int lmc_vtv_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t n_channels, int64_t channel_stride, int32_t H, int32_t W, float t_sigma,
                 int32_t niter, float step, const float* betas_host, int32_t box_enable, float box_lo, float box_hi, void* stream) {
  int rc = check_vtv_call(x_dev, out_dev, n_img, n_channels, channel_stride, H, W);
  if (rc) return rc;
  if (niter < 1 || niter > lmc::kMaxTvIters) return fail(LMC_E_INVALID, "niter %d outside 1..%d", niter, lmc::kMaxTvIters);
  if (!(t_sigma >= 0.f)) return fail(LMC_E_INVALID, "t_sigma must be >= 0 (got %g)", (double)t_sigma);
  if (!(step >= 0.f)) return fail(LMC_E_INVALID, "step must be >= 0 (0: the default 1/8)");
  if (box_enable) {
    if (box_enable != 1) return fail(LMC_E_INVALID, "box_enable must be 0 or 1 (got %d)", box_enable);
    if (!(box_lo == box_lo) || !(box_hi == box_hi)) return fail(LMC_E_INVALID, "box: a bound is NaN");
    if (!(box_lo < box_hi)) return fail(LMC_E_INVALID, "box: needs box_lo < box_hi (got [%g, %g])", (double)box_lo, (double)box_hi);
  }
  const size_t plane = sizeof(float) * (size_t)n_img * H * W;
  if (t_sigma == 0.f) {      // the prox of the zero function
    for (int ch = 0; ch < n_channels; ++ch)
      HIP_TRY(hipMemcpyAsync(out_dev + (size_t)ch * channel_stride, x_dev + (size_t)ch * channel_stride, plane, hipMemcpyDeviceToDevice, S(stream)));
    return LMC_OK;
  }
  float betas[lmc::kMaxTvIters];
  if (betas_host) std::memcpy(betas, betas_host, sizeof(float) * niter);
  else default_betas(betas, niter);
  Workspace& sc = scratch_here();
  const size_t ns = lmc::vtv_state_floats(n_img, n_channels, H, W, niter);
  HIP_TRY(sc.state[0].need(ns));
  HIP_TRY(sc.state[1].need(ns));
  HIP_TRY(lmc::launch_vtv_prox(x_dev, out_dev, n_img, n_channels, channel_stride, H, W, t_sigma, step > 0.f ? step : 0.125f, betas, niter, box_enable, box_lo,
                               box_hi, sc.state[0].p, sc.state[1].p, S(stream)));
  return LMC_OK;
}

int lmc_vtv_value(const float* x_dev, double* out_dev, int64_t n_img, int32_t n_channels, int64_t channel_stride, int32_t H, int32_t W, void* stream) {
  int rc = check_vtv_call(x_dev, out_dev, n_img, n_channels, channel_stride, H, W);
  if (rc) return rc;
  Workspace& sc = scratch_here();
  HIP_TRY(sc.vtv_part.need(lmc::vtv_value_partials(n_img, H, W)));
  HIP_TRY(lmc::launch_vtv_value(x_dev, n_img, n_channels, channel_stride, H, W, 1.0, sc.vtv_part.p, out_dev, S(stream)));
  return LMC_OK;
}

int lmc_vtv_plan(int32_t H, int32_t W, int32_t n_channels, int32_t niter, int32_t* tile_h, int32_t* tile_w, int32_t* iters_per_launch, int32_t* n_launches) {
  if (H < 1 || W < 1) return fail(LMC_E_INVALID, "bad image size %dx%d", H, W);
  if (n_channels < 1 || n_channels > LMC_MAX_CHANNELS) return fail(LMC_E_INVALID, "n_channels %d outside 1..%d", n_channels, LMC_MAX_CHANNELS);
  if (niter < 1 || niter > lmc::kMaxTvIters) return fail(LMC_E_INVALID, "niter %d outside 1..%d", niter, lmc::kMaxTvIters);
  lmc::VtvPlan pl;
  if (!lmc::vtv_plan(n_channels, niter, pl)) return fail(LMC_E_INVALID, "no plan");
  if (tile_h) *tile_h = pl.TH;
  if (tile_w) *tile_w = pl.TW;
  if (iters_per_launch) *iters_per_launch = pl.iters;
  if (n_launches) *n_launches = pl.n_launches;
  return LMC_OK;
}

int lmc_tgv_prox(const float* x_dev, float* out_dev, float* w_out_dev, int64_t n_img, int32_t H, int32_t W, float t_sigma, float alpha0, int32_t niter,
                 float step, int32_t box_enable, float box_lo, float box_hi, void* stream) {
  if (!x_dev || !out_dev || x_dev == out_dev || w_out_dev == x_dev || w_out_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || n_img > (1 << 24) || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30)
    return fail(LMC_E_INVALID, "bad shape n_img=%lld H=%d W=%d", (long long)n_img, H, W);
  if (niter < 1 || niter > LMC_MAX_TGV_ITERS) return fail(LMC_E_INVALID, "niter %d outside 1..%d", niter, LMC_MAX_TGV_ITERS);
  if (!(t_sigma >= 0.f) || !std::isfinite(t_sigma)) return fail(LMC_E_INVALID, "t_sigma must be finite and >= 0 (got %g)", (double)t_sigma);
  if (!std::isfinite(alpha0) || !(alpha0 > 0.f)) return fail(LMC_E_INVALID, "alpha0 must be finite and > 0 (got %g)", (double)alpha0);
  int rc = check_tgv_step(step);
  if (rc) return rc;
  if (box_enable) {
    if (box_enable != 1) return fail(LMC_E_INVALID, "box_enable must be 0 or 1 (got %d)", box_enable);
    if (!(box_lo == box_lo) || !(box_hi == box_hi)) return fail(LMC_E_INVALID, "box: a bound is NaN");
    if (!(box_lo < box_hi)) return fail(LMC_E_INVALID, "box: needs box_lo < box_hi (got [%g, %g])", (double)box_lo, (double)box_hi);
  }
  const size_t npx = (size_t)n_img * H * W;
  if (t_sigma == 0.f) {      // the prox of the indicator alone
    if (box_enable) HIP_TRY(lmc::launch_box_prox(LMC_PRIOR_NONE, 0, x_dev, out_dev, n_img, (int64_t)H * W, nullptr, 0, 0, 0.f, 0.f, 0.f, 0.f, 0, box_lo, box_hi, S(stream)));
    else HIP_TRY(hipMemcpyAsync(out_dev, x_dev, sizeof(float) * npx, hipMemcpyDeviceToDevice, S(stream)));
    if (w_out_dev) HIP_TRY(hipMemsetAsync(w_out_dev, 0, sizeof(float) * 2 * npx, S(stream)));
    return LMC_OK;
  }
  Workspace& sc = scratch_here();
  const size_t ns = lmc::tgv_state_floats(n_img, H, W, niter);
  HIP_TRY(sc.state[0].need(ns));
  HIP_TRY(sc.state[1].need(ns));
  HIP_TRY(lmc::launch_tgv_prox(x_dev, out_dev, w_out_dev, n_img, H, W, t_sigma, alpha0, step > 0.f ? step : lmc::kTgvStep, niter, box_enable, box_lo, box_hi,
                               sc.state[0].p, sc.state[1].p, S(stream)));
  return LMC_OK;
}

int lmc_tgv_launch_iters(void) { return lmc::kTgvLaunchIters; }

int lmc_chain_probes(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t ph, int32_t pw, void* stream) {
  if (!x_dev || !out_dev || n_img < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (ph < 1 || pw < 1 || ph > H || pw > W) return fail(LMC_E_INVALID, "probe grid %dx%d does not fit a %dx%d image", ph, pw, H, W);
  if (W > 8192) return fail(LMC_E_UNSUPPORTED, "W <= 8192 (got %d)", W);
  HIP_TRY(lmc::launch_chain_probes(x_dev, out_dev, n_img, H, W, ph, pw, S(stream)));
  return LMC_OK;
}

int lmc_pixel_histogram(const float* x_dev, int64_t C, int32_t H, int32_t W, int32_t n_bins, const float* lo_dev, const float* scale_dev,
                        uint64_t* counts_dev, void* stream) {
  if (!x_dev || !lo_dev || !scale_dev || !counts_dev || C < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (n_bins < 1 || n_bins > 62) return fail(LMC_E_INVALID, "n_bins must be 1 .. 62 (got %d)", n_bins);
  HIP_TRY(lmc::launch_pixel_hist(x_dev, C, H, W, n_bins, lo_dev, scale_dev, reinterpret_cast<unsigned long long*>(counts_dev), S(stream)));
  return LMC_OK;
}

int lmc_group_moments(const float* x_dev, int64_t C, int64_t chain_offset, int32_t H, int32_t W, int32_t n_groups, double* sum_dev, double* sumsq_dev,
                      void* stream) {
  if (!x_dev || !sum_dev || !sumsq_dev || C < 1 || chain_offset < 0 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (n_groups < 2 || n_groups > LMC_MAX_CHAIN_GROUPS) return fail(LMC_E_INVALID, "n_groups must be 2 .. %d (got %d)", LMC_MAX_CHAIN_GROUPS, n_groups);
  HIP_TRY(lmc::launch_group_moments(x_dev, C, chain_offset, H, W, n_groups, sum_dev, sumsq_dev, S(stream)));
  return LMC_OK;
}

size_t lmc_cov_sketch_workspace_bytes(int64_t C, int32_t H, int32_t W, int32_t k) { return lmc::cov_sketch_workspace_bytes(C, H, W, k); }

int lmc_cov_sketch(const float* x_dev, int64_t C, int32_t H, int32_t W, int32_t k, const float* probes_dev, const float* center_dev, double* y_dev,
                   double* s_dev, double* q_dev, void* workspace_dev, void* stream) {
  if (!x_dev || !probes_dev || !y_dev || !s_dev || !q_dev || !workspace_dev || C < 1 || H < 1 || W < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (k < 1 || k > LMC_MAX_COV_PROBES) return fail(LMC_E_INVALID, "k must be 1 .. %d (got %d)", LMC_MAX_COV_PROBES, k);
  if (reinterpret_cast<uintptr_t>(workspace_dev) & 15) return fail(LMC_E_INVALID, "the workspace must be 16-byte aligned");
  HIP_TRY(lmc::launch_cov_sketch(x_dev, C, H, W, k, probes_dev, center_dev, y_dev, s_dev, q_dev, workspace_dev, S(stream)));
  return LMC_OK;
}

int lmc_dual_project(const float* y_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, float radius,
                     int32_t isotropic, void* stream) {
  if (!y_dev || !out_dev) return fail(LMC_E_INVALID, "NULL pointer");
  if (n_img < 1 || H < 1 || W < 1 || !(radius > 0.f)) return fail(LMC_E_INVALID, "bad shape or radius");
  HIP_TRY(lmc::launch_dual_project(y_dev, out_dev, n_img, H, W, radius, isotropic, S(stream)));
  return LMC_OK;
}

int lmc_prox_elementwise(int32_t kind, const float* x_dev, float* out_dev, int64_t n, const float* params_host,
                         int32_t n_params, void* stream) {
  static const int need[] = {1, 2, 1, 1, 1, 1, 1, 2, 1, 1, 2, 1, 1, 2, 1};
  if (kind < 0 || kind > LMC_EPROX_LAPLACE_CONJ) return fail(LMC_E_INVALID, "unknown elementwise prox %d", kind);
  if (!x_dev || !out_dev || n < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (n_params != need[kind] || !params_host)
    return fail(LMC_E_INVALID, "elementwise prox %d takes %d parameter(s), got %d", kind, need[kind], n_params);
  const float p0 = params_host[0], p1 = n_params > 1 ? params_host[1] : 0.f;
  if (!eprox_params_ok(kind, p0, p1)) return fail(LMC_E_INVALID, "elementwise prox %d: negative (or NaN) weight %g, %g", kind, (double)p0, (double)p1);
  HIP_TRY(lmc::launch_eprox(kind, x_dev, out_dev, n, p0, p1, S(stream)));
  return LMC_OK;
}
}  // extern "C"
