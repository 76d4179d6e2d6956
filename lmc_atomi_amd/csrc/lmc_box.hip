// Box-constrained separable priors: for g separable (none, l2, l1, the closed forms of prox.py) the prox of g + the indicator of [lo, hi] is the clamp
// of the prox of g, pixel by pixel (a convex function of one variable restricted to an interval: its minimiser is the free one moved to the nearest end).
// One elementwise launch forms it; the fused step consumes it as a ready-made prox (StepArgs::prox_ext, prior NONE) -- the route array-valued epsg takes
// (launch_prior_prox_scaled, lmc_ops.hip), and with an array-valued epsg the same launch serves both.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

// scale == NULL: p0 / p1 are the step's own parameters (StepArgs::prior_p0 / prior_p1: l2 the factor 1 / (1 + t sigma), l1 the threshold, EPROX the closed
// form's parameters already scaled).  scale != NULL: t(c, i) = pt * scale[c * cs + i * ps] and the parameters are formed here, as prior_prox_scaled_kernel does.
__global__ __launch_bounds__(256) void box_prior_prox_kernel(int prior, int kind, const float* __restrict__ x, float* __restrict__ out, size_t img, size_t n,
                                                            const float* __restrict__ scale, size_t cs, size_t ps, float pt, float sigma, float p0,
                                                            float p1, int mask, float lo, float hi) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    float o = v;
    if (scale) {
      const size_t c = i / img, px = i - c * img;
      const float t = pt * scale[c * cs + px * ps];
      if (prior == LMC_PRIOR_L2) o = v * (1.f / (1.f + t * sigma));
      else if (prior == LMC_PRIOR_L1) o = soft(v, t * sigma);
      else if (prior == LMC_PRIOR_EPROX) o = eprox(kind, v, EproxParams{(mask & 1) ? t * p0 : p0, (mask & 2) ? t * p1 : p1});
    } else {
      if (prior == LMC_PRIOR_L2) o = v * p0;
      else if (prior == LMC_PRIOR_L1) o = soft(v, p0);
      else if (prior == LMC_PRIOR_EPROX) o = eprox(kind, v, EproxParams{p0, p1});
    }
    out[i] = __builtin_amdgcn_fmed3f(o, lo, hi);
  }
}

hipError_t launch_box_prox(int prior, int kind, const float* x, float* out, int64_t n_chains, int64_t img, const float* scale, int64_t cs, int64_t ps,
                           float pt, float sigma, float p0, float p1, int mask, float lo, float hi, hipStream_t st) {
  if (prior != LMC_PRIOR_NONE && prior != LMC_PRIOR_L2 && prior != LMC_PRIOR_L1 && prior != LMC_PRIOR_EPROX) return hipErrorInvalidConfiguration;
  if (!(lo < hi) || !x || !out) return hipErrorInvalidValue;
  const size_t n = (size_t)n_chains * (size_t)img;
  size_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(box_prior_prox_kernel, dim3((unsigned)blocks), dim3(256), 0, st, prior, kind, x, out, (size_t)img, n, scale, (size_t)cs, (size_t)ps, pt,
                     sigma, p0, p1, mask, lo, hi);
  return hipGetLastError();
}

}  // namespace lmc
