// The accumulators of a sampler handle (lmc_accum.h): what a kept iterate is reduced into, and the entry points that configure, read and reset them.
#include <initializer_list>

#include "lmc_host.h"

using namespace lmc::host;

namespace lmc::host {

static void drop(std::initializer_list<void*> ps) {
  for (void* p : ps) if (p) (void)hipFree(p);
}
// A set call whose device allocation failed (its buffers are released already): the status says why.
static int alloc_failed(const char* what, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? LMC_E_NOMEM : LMC_E_HIP, "%s allocation failed: %s", what, hipGetErrorString(e));
}

void BlockMoments::release() { drop({buf}); *this = BlockMoments{}; }
void Histogram::release() { drop({counts, lo, scale, packed}); *this = Histogram{}; }
void ChainGroups::release() { drop({sums, packed}); *this = ChainGroups{}; }
void CovSketch::release() { drop({buf, probes, center, ws}); *this = CovSketch{}; }

hipError_t Accumulators::alloc(int C_, int64_t chain_offset_, int H_, int W_) {
  C = C_; chain_offset = chain_offset_; H = H_; W = W_;
  const size_t mb = sizeof(double) * pixels();
  hipError_t e = hipMalloc(&s1, mb);
  if (e == hipSuccess) e = hipMalloc(&s2, mb);
  if (e == hipSuccess) e = hipMemset(s1, 0, mb);
  if (e == hipSuccess) e = hipMemset(s2, 0, mb);
  return e;
}

void Accumulators::release() {
  drop({s1, s2, packed});
  s1 = s2 = packed = nullptr;
  blocks.release(); hist.release(); groups.release(); cov.release();
}

int Accumulators::reset(hipStream_t st) {
  HIP_TRY(hipMemsetAsync(s1, 0, sizeof(double) * pixels(), st));
  HIP_TRY(hipMemsetAsync(s2, 0, sizeof(double) * pixels(), st));
  if (blocks.buf) HIP_TRY(hipMemsetAsync(blocks.buf, 0, sizeof(double) * blocks.elems(H, W), st));
  if (hist.counts) HIP_TRY(hipMemsetAsync(hist.counts, 0, sizeof(unsigned long long) * hist.elems(H, W), st));
  if (groups.sums) HIP_TRY(hipMemsetAsync(groups.sums, 0, sizeof(double) * groups.elems(H, W), st));
  if (cov.buf) HIP_TRY(hipMemsetAsync(cov.buf, 0, sizeof(double) * cov.elems(H, W), st));
  count = 0;
  return LMC_OK;
}

hipError_t Accumulators::reduce_more(hipError_t e, const float* x, hipStream_t st) {
  if (e == hipSuccess && hist.counts) e = lmc::launch_pixel_hist(x, C, H, W, hist.bins, hist.lo, hist.scale, hist.counts, st);
  if (e == hipSuccess && groups.sums) e = lmc::launch_group_moments(x, C, chain_offset, H, W, groups.n, groups.sums, groups.sums + groups.elems(H, W) / 2, st);
  if (e == hipSuccess && cov.buf) {
    const size_t ny = cov.y_elems(H, W);
    e = lmc::launch_cov_sketch(x, C, H, W, cov.k, cov.probes, cov.center, cov.buf, cov.buf + ny, cov.buf + ny + cov.k, cov.ws, st);
  }
  return e;
}

hipError_t Accumulators::reduce(const float* x, hipStream_t st) {
  return reduce_more(blocks.buf ? lmc::launch_moments_ms(x, C, H, W, s1, s2, blocks.scales, st) : lmc::launch_moments(x, C, H, W, s1, s2, st), x, st);
}

hipError_t Accumulators::reduce_bg(const float* x, int n_wg, hipStream_t st) {
  return reduce_more(blocks.buf ? lmc::launch_moments_ms_bg(x, C, H, W, s1, s2, blocks.scales, n_wg, st) : lmc::launch_moments_bg(x, C, H, W, s1, s2, n_wg, st), x, st);
}

int accum_get_moments(const Accumulators& a, int moments, double* sum_dev, double* sumsq_dev, uint64_t* count, hipStream_t st) {
  if (!moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  const size_t mb = sizeof(double) * a.pixels();
  if (sum_dev) HIP_TRY(hipMemcpyAsync(sum_dev, a.s1, mb, hipMemcpyDeviceToDevice, st));
  if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev, a.s2, mb, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (count) *count = a.count;
  return LMC_OK;
}

int accum_set_chain_groups(Accumulators& a, int moments, int32_t n_groups) {
  if (n_groups != 0 && (n_groups < 2 || n_groups > LMC_MAX_CHAIN_GROUPS))
    return fail(LMC_E_INVALID, "n_groups must be 0 or 2 .. %d (got %d)", LMC_MAX_CHAIN_GROUPS, n_groups);
  if (!moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  if (a.count != 0) return fail(LMC_E_STATE, "the chain groups change only while the accumulators are empty (after create or a reset of the moments)");
  HIP_TRY(hipDeviceSynchronize());     // nothing of earlier groups is in flight when their buffers go
  ChainGroups& g = a.groups;
  g.release();
  if (!n_groups) return LMC_OK;
  g.n = n_groups;
  const size_t nd = g.elems(a.H, a.W);
  hipError_t e = hipMalloc(&g.sums, sizeof(double) * nd);
  if (e == hipSuccess) e = hipMemset(g.sums, 0, sizeof(double) * nd);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { g.release(); return alloc_failed("chain-group", e); }
  return LMC_OK;
}

int accum_get_group_moments(const Accumulators& a, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, hipStream_t st) {
  if (!a.groups.sums) return fail(LMC_E_INVALID, "the sampler has no chain groups (set them with its set_chain_groups call)");
  const size_t n = a.groups.elems(a.H, a.W) / 2;
  if (sum_dev) HIP_TRY(hipMemcpyAsync(sum_dev, a.groups.sums, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev, a.groups.sums + n, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (counts_host) a.group_counts(counts_host);
  return LMC_OK;
}

}  // namespace lmc::host

extern "C" {

int lmc_sampler_get_moments(lmc_sampler* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_get_moments(s->acc, s->moments, sum_dev, sumsq_dev, count, S(stream));
}

int lmc_sampler_reset_moments(lmc_sampler* s, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  return s->acc.reset(S(stream));
}

// ---- multi-scale moments: sum b and sum b^2 of the block sums b of every kept sample, for scales out of {2, 4, 8, 16} ----
int lmc_sampler_set_moment_scales(lmc_sampler* s, int32_t n_scales, const int32_t* scales) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (n_scales < 0 || n_scales > 4 || (n_scales > 0 && !scales)) return fail(LMC_E_INVALID, "n_scales must be 0 .. 4 (distinct scales out of 2, 4, 8, 16)");
  BlockMoments asked;
  for (int i = 0; i < n_scales; ++i) {
    const int k = BlockMoments::index(scales[i]);
    if (k < 0) return fail(LMC_E_INVALID, "moment scale %d: the scales are 2, 4, 8 and 16", scales[i]);
    if (asked.on[k]) return fail(LMC_E_INVALID, "moment scale %d given twice", scales[i]);
    asked.on[k] = true;
  }
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  Accumulators& a = s->acc;
  if (a.count != 0) return fail(LMC_E_STATE, "the moment scales change only while the accumulators are empty (after create or lmc_sampler_reset_moments)");
  BlockMoments& b = a.blocks;
  if (b.buf) HIP_TRY(hipFree(b.buf));
  b = asked;
  const size_t total = b.elems(a.H, a.W);
  if (!total) return LMC_OK;
  hipError_t e = hipMalloc(&b.buf, sizeof(double) * total);
  if (e == hipSuccess) e = hipMemset(b.buf, 0, sizeof(double) * total);
  if (e != hipSuccess) { b.release(); return alloc_failed("block-moment", e); }
  size_t off = 0;
  for (int k = 0; k < 4; ++k)
    if (b.on[k]) { b.scales.s2[k] = b.buf + off; off += BlockMoments::blocks(a.H, a.W, k); }
  return LMC_OK;
}

int lmc_sampler_get_block_moments(lmc_sampler* s, int32_t scale, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  const Accumulators& a = s->acc;
  const int k = BlockMoments::index(scale);
  if (k < 0 || !a.blocks.scales.s2[k]) return fail(LMC_E_INVALID, "moment scale %d is not enabled (lmc_sampler_set_moment_scales)", scale);
  if (sum_dev) HIP_TRY(lmc::launch_block_sums(a.s1, a.H, a.W, scale, sum_dev, S(stream)));
  if (sumsq_dev) HIP_TRY(hipMemcpyAsync(sumsq_dev, a.blocks.scales.s2[k], sizeof(double) * BlockMoments::blocks(a.H, a.W, k), hipMemcpyDeviceToDevice, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  if (count) *count = a.count;
  return LMC_OK;
}

// ---- pixel histograms: counts [n_bins + 2][H][W] of the kept samples, rows by t = (x - lo) * scale (lmc_pixel_hist.hip) ----
int lmc_sampler_set_histogram(lmc_sampler* s, int32_t n_bins, const float* lo_dev, const float* scale_dev) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (n_bins < 0 || n_bins > 62) return fail(LMC_E_INVALID, "n_bins must be 0 .. 62 (got %d)", n_bins);
  if (n_bins > 0 && (!lo_dev || !scale_dev)) return fail(LMC_E_INVALID, "NULL lo / scale array with n_bins > 0");
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  Accumulators& a = s->acc;
  if (a.count != 0) return fail(LMC_E_STATE, "the histogram changes only while the accumulators are empty (after create or lmc_sampler_reset_moments)");
  HIP_TRY(hipDeviceSynchronize());     // nothing of an earlier histogram is in flight when its buffers go
  Histogram& h = a.hist;
  h.release();
  if (!n_bins) return LMC_OK;
  h.bins = n_bins;
  const size_t img = a.pixels(), nc = h.elems(a.H, a.W);
  hipError_t e = hipMalloc(&h.counts, sizeof(unsigned long long) * nc);
  if (e == hipSuccess) e = hipMalloc(&h.lo, sizeof(float) * img);
  if (e == hipSuccess) e = hipMalloc(&h.scale, sizeof(float) * img);
  if (e == hipSuccess) e = hipMemset(h.counts, 0, sizeof(unsigned long long) * nc);
  if (e == hipSuccess) e = hipMemcpy(h.lo, lo_dev, sizeof(float) * img, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(h.scale, scale_dev, sizeof(float) * img, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { h.release(); return alloc_failed("histogram", e); }
  return LMC_OK;
}

int lmc_sampler_get_histogram(lmc_sampler* s, uint64_t* counts_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  const Accumulators& a = s->acc;
  if (!a.hist.counts) return fail(LMC_E_INVALID, "the sampler has no histogram (lmc_sampler_set_histogram)");
  if (counts_dev) HIP_TRY(hipMemcpyAsync(counts_dev, a.hist.counts, sizeof(unsigned long long) * a.hist.elems(a.H, a.W), hipMemcpyDeviceToDevice, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  if (count) *count = a.count;
  return LMC_OK;
}

// ---- chain-group moments: A, B [n_groups][H][W] = sum x, sum x^2 of the kept samples by chain group (lmc_group_moments.hip) ----
int lmc_sampler_set_chain_groups(lmc_sampler* s, int32_t n_groups) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_set_chain_groups(s->acc, s->moments, n_groups);
}

int lmc_sampler_get_group_moments(lmc_sampler* s, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_get_group_moments(s->acc, sum_dev, sumsq_dev, counts_host, S(stream));
}

// ---- covariance sketch: Y [k][H][W], s [k], Q [k][k] of the kept samples against k probe images (lmc_cov_sketch.hip) ----
int lmc_sampler_set_cov_sketch(lmc_sampler* s, int32_t k, const float* probes_dev, const float* center_dev) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (k < 0 || k > LMC_MAX_COV_PROBES) return fail(LMC_E_INVALID, "k must be 0 .. %d (got %d)", LMC_MAX_COV_PROBES, k);
  if (k > 0 && !probes_dev) return fail(LMC_E_INVALID, "NULL probe array with k > 0");
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  Accumulators& a = s->acc;
  if (a.count != 0) return fail(LMC_E_STATE, "the covariance sketch changes only while the accumulators are empty (after create or lmc_sampler_reset_moments)");
  HIP_TRY(hipDeviceSynchronize());     // nothing of an earlier sketch is in flight when its buffers go
  CovSketch& c = a.cov;
  c.release();
  if (!k) return LMC_OK;
  c.k = k;
  const size_t img = a.pixels(), nd = c.elems(a.H, a.W);
  hipError_t e = hipMalloc(&c.buf, sizeof(double) * nd);
  if (e == hipSuccess) e = hipMalloc(&c.probes, sizeof(float) * k * img);
  if (e == hipSuccess && center_dev) e = hipMalloc(&c.center, sizeof(float) * img);
  if (e == hipSuccess) e = hipMalloc(&c.ws, lmc::cov_sketch_workspace_bytes(a.C, a.H, a.W, k));
  if (e == hipSuccess) e = hipMemset(c.buf, 0, sizeof(double) * nd);
  if (e == hipSuccess) e = hipMemcpy(c.probes, probes_dev, sizeof(float) * k * img, hipMemcpyDeviceToDevice);
  if (e == hipSuccess && center_dev) e = hipMemcpy(c.center, center_dev, sizeof(float) * img, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { c.release(); return alloc_failed("covariance-sketch", e); }
  return LMC_OK;
}

int lmc_sampler_get_cov_sketch(lmc_sampler* s, double* y_dev, double* s_dev, double* q_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  const Accumulators& a = s->acc;
  if (!a.cov.buf) return fail(LMC_E_INVALID, "the sampler has no covariance sketch (lmc_sampler_set_cov_sketch)");
  const size_t k = (size_t)a.cov.k, ny = a.cov.y_elems(a.H, a.W);
  if (y_dev) HIP_TRY(hipMemcpyAsync(y_dev, a.cov.buf, sizeof(double) * ny, hipMemcpyDeviceToDevice, S(stream)));
  if (s_dev) HIP_TRY(hipMemcpyAsync(s_dev, a.cov.buf + ny, sizeof(double) * k, hipMemcpyDeviceToDevice, S(stream)));
  if (q_dev) HIP_TRY(hipMemcpyAsync(q_dev, a.cov.buf + ny + k, sizeof(double) * k * k, hipMemcpyDeviceToDevice, S(stream)));
  HIP_TRY(hipStreamSynchronize(S(stream)));
  if (count) *count = a.count;
  return LMC_OK;
}

}  // extern "C"
