// SAPG estimation of the prior weight theta = prior_sigma by marginal maximum likelihood (definition: include/lmc_atomi.h; Vidal, De Bortoli,
// Pereyra, Durmus 2020, Algorithm 1): one sampler iteration alternates with one projected gradient step on theta, and the gradient needs only
// g(x_c) of the current samples.
//   prior_stat_kernel    stat[i] = g(x_i) with weight 1: one streaming read of the state, no data term and no LDS tile.  The per-pixel terms are
//                        those of energy_kernel (lmc_ops.hip), fp32, summed in float64.  The image index is blockIdx.x (any image count), an
//                        image is read by `nseg` workgroups (blockIdx.y), each a band of rows; a thread's partial sum, the wave shuffles and the
//                        per-wave slots are all in a fixed order and nothing is added atomically, so two runs give the same bits.
//                        16 bytes per lane where W % 4 == 0 and the array is 16-byte aligned, a plain form for any W.
//   sapg_update_kernel   one workgroup: gbar = the float64 mean of stat[C] in a fixed order, the update of lmc_sapg_update.h, the device traces,
//                        and (theta_{n+1}, gbar) into a pinned host-mapped pair that the host reads after the event recorded behind the launch.
#include <cmath>

#include "lmc_device.h"
#include "lmc_host.h"
#include "lmc_sapg_update.h"

namespace lmc {

namespace {
constexpr int kStatThreads = 256;

// |detail coefficients| of the 3-level Haar transform of one 8 x 8 block held in registers: the forward butterflies of haar_l1_kernel (lmc_ops.hip),
// MODE 1, in its order
__device__ __forceinline__ float haar8_detail_l1(float (&v)[8][8]) {
  float dsum = 0.f;
#pragma unroll
  for (int s = 1; s <= 4; s <<= 1) {
#pragma unroll
    for (int i = 0; i < 8; i += 2 * s)
#pragma unroll
      for (int j = 0; j < 8; j += 2 * s) {
        const float a = v[i][j], b = v[i][j + s], cc = v[i + s][j], d = v[i + s][j + s];
        const float ll = 0.5f * (a + b + cc + d), lh = 0.5f * (a - b + cc - d), hl = 0.5f * (a + b - cc - d), hh = 0.5f * (a - b - cc + d);
        v[i][j] = ll;
        dsum += fabsf(lh) + fabsf(hl) + fabsf(hh);
      }
  }
  return dsum;
}

// the term of one pixel from its value, the value below (dx = below - v) and the value to the right (dy = right - v); at the last row / column
// the caller passes v itself, so the difference is the zero energy_kernel uses there
template <int PRIOR>
__device__ __forceinline__ double pixel_term(float v, float below, float right) {
  if (PRIOR == LMC_PRIOR_TV_ISO) {
    const float dx = below - v, dy = right - v;
    return (double)sqrtf(fmaf(dx, dx, dy * dy));
  }
  if (PRIOR == LMC_PRIOR_TV_ANISO) return (double)fabsf(below - v) + (double)fabsf(right - v);
  if (PRIOR == LMC_PRIOR_L1) return (double)fabsf(v);
  return 0.5 * (double)v * (double)v;      // LMC_PRIOR_L2
}
}  // namespace

// out[blockIdx.x * gridDim.y + blockIdx.y] = the sum of the terms of rows [blockIdx.y * rows_per_seg, +rows_per_seg) of image blockIdx.x
template <int PRIOR, bool VEC>
__global__ __launch_bounds__(kStatThreads) void prior_stat_kernel(const float* __restrict__ x, int H, int W, int rows_per_seg, double* __restrict__ out) {
  __shared__ double scratch[kStatThreads / kWave];
  const float* __restrict__ xi = x + (size_t)blockIdx.x * ((size_t)H * W);
  const unsigned r0 = blockIdx.y * (unsigned)rows_per_seg;
  const unsigned r1 = min(r0 + (unsigned)rows_per_seg, (unsigned)H);
  const unsigned uH = (unsigned)H, uW = (unsigned)W;
  double acc = 0.0;
  if (PRIOR == LMC_PRIOR_HAAR_L1) {          // one thread = one 8 x 8 block; H, W, rows_per_seg multiples of 8
    const unsigned nbx = uW >> 3;
    const unsigned b0 = (r0 >> 3) * nbx, b1 = (r1 >> 3) * nbx;
    for (unsigned bi = b0 + threadIdx.x; bi < b1; bi += kStatThreads) {
      const unsigned by = bi / nbx, bx = bi - by * nbx;
      const float* src = xi + (size_t)(by * 8u) * uW + bx * 8u;
      float v[8][8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        if (VEC) {
          const float4 lo = *reinterpret_cast<const float4*>(src + (size_t)r * uW);
          const float4 hi = *reinterpret_cast<const float4*>(src + (size_t)r * uW + 4);
          v[r][0] = lo.x; v[r][1] = lo.y; v[r][2] = lo.z; v[r][3] = lo.w; v[r][4] = hi.x; v[r][5] = hi.y; v[r][6] = hi.z; v[r][7] = hi.w;
        } else {
#pragma unroll
          for (int c = 0; c < 8; ++c) v[r][c] = src[(size_t)r * uW + c];
        }
      }
      acc += (double)haar8_detail_l1(v);
    }
  } else if (VEC) {                          // one thread = four pixels of a row; W % 4 == 0, x 16-byte aligned
    const unsigned w4 = uW >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xi);
    constexpr bool tv = PRIOR == LMC_PRIOR_TV_ISO || PRIOR == LMC_PRIOR_TV_ANISO;
#pragma unroll 2
    for (unsigned q = r0 * w4 + threadIdx.x; q < r1 * w4; q += kStatThreads) {
      const float4 v = x4[q];
      float4 b = v;
      float nx = v.w;
      if (tv) {
        const unsigned r = q / w4, g = q - r * w4;
        if (r + 1u < uH) b = x4[q + w4];
        if (g + 1u < w4) nx = xi[4u * (size_t)q + 4u];
      }
      acc += pixel_term<PRIOR>(v.x, b.x, v.y);
      acc += pixel_term<PRIOR>(v.y, b.y, v.z);
      acc += pixel_term<PRIOR>(v.z, b.z, v.w);
      acc += pixel_term<PRIOR>(v.w, b.w, nx);
    }
  } else {
    constexpr bool tv = PRIOR == LMC_PRIOR_TV_ISO || PRIOR == LMC_PRIOR_TV_ANISO;
    for (unsigned p = r0 * uW + threadIdx.x; p < r1 * uW; p += kStatThreads) {
      const float v = xi[p];
      float b = v, nx = v;
      if (tv) {
        const unsigned r = p / uW, c = p - r * uW;
        if (r + 1u < uH) b = xi[(size_t)p + uW];
        if (c + 1u < uW) nx = xi[(size_t)p + 1u];
      }
      acc += pixel_term<PRIOR>(v, b, nx);
    }
  }
  const double tot = block_sum(acc, scratch);
  if (threadIdx.x == 0) out[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = tot;
}

// stat[i] = part[i][0] + part[i][1] + ... in that order
__global__ __launch_bounds__(256) void prior_stat_sum_kernel(const double* __restrict__ part, int64_t n_img, int nseg, double* __restrict__ stat) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_img) return;
  double a = 0.0;
  for (int k = 0; k < nseg; ++k) a += part[(size_t)i * nseg + k];
  stat[i] = a;
}

__global__ __launch_bounds__(256) void sapg_update_kernel(const double* __restrict__ stat, int C, SapgParams P, long long n, double theta,
                                                          double* __restrict__ theta_trace, double* __restrict__ gbar_trace,
                                                          double* __restrict__ host2) {
  __shared__ double scratch[256 / kWave];
  double a = 0.0;
  for (int i = threadIdx.x; i < C; i += 256) a += stat[i];
  const double tot = block_sum(a, scratch);
  if (threadIdx.x == 0) {
    const double gbar = tot / (double)C;
    const double next = sapg_next_theta(P, n, theta, gbar);
    theta_trace[n + 1] = next;
    gbar_trace[n] = gbar;
    host2[0] = next;
    host2[1] = gbar;
    __threadfence_system();
  }
}

namespace {
// rows per workgroup so that about 2048 workgroups read the stack: bands of at least 8 rows, a multiple of 8 (the Haar blocks)
int stat_rows_per_segment(int64_t n_img, int H) {
  int64_t want = n_img >= 2048 ? 1 : (2048 + n_img - 1) / n_img;
  const int64_t most = ((int64_t)H + 7) / 8;
  if (want > most) want = most;
  if (want > 65535) want = 65535;
  const int64_t rows = (((int64_t)H + want - 1) / want + 7) / 8 * 8;
  return (int)rows;
}

template <int PRIOR>
void stat_launch(const float* x, unsigned n, int nseg, int H, int W, int rps, bool vec, double* out, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((prior_stat_kernel<PRIOR, true>), dim3(n, nseg), dim3(kStatThreads), 0, st, x, H, W, rps, out);
  else hipLaunchKernelGGL((prior_stat_kernel<PRIOR, false>), dim3(n, nseg), dim3(kStatThreads), 0, st, x, H, W, rps, out);
}
}  // namespace

int prior_stat_segments(int64_t n_img, int H) {
  const int rps = stat_rows_per_segment(n_img, H);
  return (H + rps - 1) / rps;
}

hipError_t launch_prior_stat(const float* x, int64_t n_img, int H, int W, int prior_kind, double* stat, double* part, hipStream_t st) {
  if (!x || !stat || n_img < 1 || H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30)) return hipErrorInvalidValue;
  if (prior_kind == LMC_PRIOR_HAAR_L1 && ((H & 7) || (W & 7))) return hipErrorInvalidValue;
  const int rps = stat_rows_per_segment(n_img, H), nseg = (H + rps - 1) / rps;
  if (nseg > 1 && !part) return hipErrorInvalidValue;
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  double* out = nseg > 1 ? part : stat;
  const size_t img = (size_t)H * W;
  const int64_t chunk = (int64_t)1 << 30;      // images per launch (gridDim.x)
  for (int64_t i0 = 0; i0 < n_img; i0 += chunk) {
    const unsigned n = (unsigned)((n_img - i0) < chunk ? (n_img - i0) : chunk);
    const float* xc = x + (size_t)i0 * img;
    double* oc = out + (size_t)i0 * nseg;
    switch (prior_kind) {
      case LMC_PRIOR_L2: stat_launch<LMC_PRIOR_L2>(xc, n, nseg, H, W, rps, vec, oc, st); break;
      case LMC_PRIOR_L1: stat_launch<LMC_PRIOR_L1>(xc, n, nseg, H, W, rps, vec, oc, st); break;
      case LMC_PRIOR_TV_ISO: stat_launch<LMC_PRIOR_TV_ISO>(xc, n, nseg, H, W, rps, vec, oc, st); break;
      case LMC_PRIOR_TV_ANISO: stat_launch<LMC_PRIOR_TV_ANISO>(xc, n, nseg, H, W, rps, vec, oc, st); break;
      case LMC_PRIOR_HAAR_L1: stat_launch<LMC_PRIOR_HAAR_L1>(xc, n, nseg, H, W, rps, vec, oc, st); break;
      default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (nseg > 1) {
    hipLaunchKernelGGL(prior_stat_sum_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, n_img, nseg, stat);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_sapg_update(const double* stat, int C, const SapgParams& P, long long n, double theta, double* theta_trace, double* gbar_trace,
                              double* host2, hipStream_t st) {
  if (!stat || C < 1 || n < 0 || !theta_trace || !gbar_trace || !host2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sapg_update_kernel, dim3(1), dim3(256), 0, st, stat, C, P, n, theta, theta_trace, gbar_trace, host2);
  return hipGetLastError();
}

}  // namespace lmc

using namespace lmc::host;

namespace {
// d and k of the table in include/lmc_atomi.h; false: the prior has no statistic
bool sapg_dimension(int prior_kind, int H, int W, int levels, double* d, double* k) {
  const double n = (double)H * (double)W;
  switch (prior_kind) {
    case LMC_PRIOR_L1: *d = n; *k = 1.0; return true;
    case LMC_PRIOR_L2: *d = n; *k = 2.0; return true;
    case LMC_PRIOR_TV_ISO: case LMC_PRIOR_TV_ANISO: *d = n - 1.0; *k = 1.0; return true;
    case LMC_PRIOR_HAAR_L1: *d = n - (double)(H / 8) * (double)(W / 8); *k = 1.0; return true;
    case LMC_PRIOR_WAVELET_L1: *d = n - (double)(H >> levels) * (double)(W >> levels); *k = 1.0; return true;
    default: return false;
  }
}

// the part of an lmc_problem the statistic and its dimension read
int check_stat_problem(const lmc_problem* p) {
  if (!p) return fail(LMC_E_INVALID, "lmc_problem is NULL");
  if (p->struct_size != sizeof(lmc_problem))
    return fail(LMC_E_INVALID, "lmc_problem.struct_size %u != %zu (ABI mismatch)", p->struct_size, sizeof(lmc_problem));
  if (p->H < 1 || p->W < 1 || (int64_t)p->H * p->W > (int64_t)1 << 30) return fail(LMC_E_INVALID, "bad image size %dx%d", p->H, p->W);
  if (p->prior_kind == LMC_PRIOR_TGV)
    return fail(LMC_E_UNSUPPORTED, "LMC_PRIOR_TGV has no statistic: its value g(x) is a minimisation over the auxiliary field and is not built");
  if (p->prior_kind < LMC_PRIOR_NONE || p->prior_kind > LMC_PRIOR_WAVELET_L1) return fail(LMC_E_INVALID, "unknown prior_kind %d", p->prior_kind);
  if (p->prior_kind == LMC_PRIOR_NONE || p->prior_kind == LMC_PRIOR_EPROX)
    return fail(LMC_E_UNSUPPORTED, "prior_kind %d has no value g(x): no statistic", p->prior_kind);
  if (p->prior_kind == LMC_PRIOR_HAAR_L1 && ((p->H & 7) || (p->W & 7)))
    return fail(LMC_E_UNSUPPORTED, "the Haar-l1 prior needs H and W to be multiples of 8 (got %dx%d)", p->H, p->W);
  if (p->prior_kind == LMC_PRIOR_WAVELET_L1 && !lmc::wavelet_shape_ok(p->H, p->W, p->eprox_kind, p->tv_niter))
    return fail(LMC_E_INVALID, "LMC_PRIOR_WAVELET_L1: a %dx%d image does not take %d levels (tv_niter) of db%d (eprox_kind)", p->H, p->W, p->tv_niter, p->eprox_kind);
  return LMC_OK;
}

int check_sapg_config(const lmc_sapg_config* c) {
  if (!c) return fail(LMC_E_INVALID, "lmc_sapg_config is NULL");
  if (c->struct_size != sizeof(lmc_sapg_config))
    return fail(LMC_E_INVALID, "lmc_sapg_config.struct_size %u != %zu (ABI mismatch)", c->struct_size, sizeof(lmc_sapg_config));
  if (!std::isfinite(c->theta_min) || !std::isfinite(c->theta_max) || !std::isfinite(c->theta0) || !(c->theta_min > 0.0) ||
      !(c->theta_min <= c->theta0) || !(c->theta0 <= c->theta_max))
    return fail(LMC_E_INVALID, "need finite 0 < theta_min <= theta0 <= theta_max (got %g, %g, %g)", c->theta_min, c->theta0, c->theta_max);
  if (!std::isfinite(c->dim_eff) || c->dim_eff < 0.0) return fail(LMC_E_INVALID, "dim_eff must be finite and >= 0 (0 = the default)");
  if (!std::isfinite(c->step_scale) || !(c->step_scale > 0.0)) return fail(LMC_E_INVALID, "step_scale must be finite and > 0");
  if (!(c->step_exponent > 0.5) || !(c->step_exponent <= 1.0)) return fail(LMC_E_INVALID, "step_exponent must be in (0.5, 1]");
  if (c->warmup_iters < 0) return fail(LMC_E_INVALID, "warmup_iters must be >= 0");
  if (c->n_updates < 1) return fail(LMC_E_INVALID, "n_updates must be >= 1");
  if (c->iters_per_update < 1) return fail(LMC_E_INVALID, "iters_per_update must be >= 1");
  if (c->average_from < 0 || c->average_from >= c->n_updates) return fail(LMC_E_INVALID, "average_from must be in 0 .. n_updates - 1");
  return LMC_OK;
}

lmc::SapgParams sapg_params(const lmc_sapg_config& c, double d, double k) {
  return lmc::SapgParams{d, k, c.step_scale, c.step_exponent, c.theta_min, c.theta_max};
}

// the buffers of lmc_sampler_sapg in the handle: statistic + partial sums, device traces, the mapped pair, the event
int sapg_buffers(lmc_sampler* s, int n_updates) {
  const size_t C = (size_t)s->C;
  if (!s->sapg_stat) HIP_TRY(s->own.alloc(&s->sapg_stat, C * (1 + (size_t)lmc::prior_stat_segments(s->C, s->prob.H)), false));
  const size_t need = 2 * (size_t)n_updates + 1;
  if (s->sapg_trace_n < need) {
    s->own.drop(s->sapg_trace);
    s->sapg_trace_n = 0;
    HIP_TRY(s->own.alloc(&s->sapg_trace, need, false));
    s->sapg_trace_n = need;
  }
  if (!s->sapg_host) {
    HIP_TRY(s->own.pinned(&s->sapg_host, 2, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&s->sapg_host_dev), s->sapg_host, 0));
  }
  if (!s->sapg_ev) HIP_TRY(s->own.event(&s->sapg_ev, hipEventDisableTiming));
  return LMC_OK;
}

int sapg_loop(lmc_sampler* s, const lmc_sapg_config& c, const lmc::SapgParams& P, const float* noise_dev, double* theta_trace_host,
              double* gbar_trace_host, double* theta_bar, hipStream_t st) {
  const size_t per_iter = (size_t)s->C * s->prob.H * s->prob.W;
  int rc = lmc_sampler_set_prior_sigma(s, (float)c.theta0);
  if (rc) return rc;
  if (c.warmup_iters > 0) {
    rc = lmc_sampler_step(s, c.warmup_iters, noise_dev, st);
    if (rc) return rc;
  }
  const float* noise = noise_dev ? noise_dev + (size_t)c.warmup_iters * per_iter : nullptr;
  double* theta_trace = s->sapg_trace;                       // [n_updates + 1]; entry 0 is the host's theta0
  double* gbar_trace = s->sapg_trace + c.n_updates + 1;      // [n_updates]
  double* part = s->sapg_stat + s->C;
  double theta = c.theta0, sum = 0.0;
  for (int n = 0; n < c.n_updates; ++n) {
    rc = lmc_sampler_step(s, c.iters_per_update, noise ? noise + (size_t)n * c.iters_per_update * per_iter : nullptr, st);
    if (rc) return rc;
    if (s->prob.wav.on)      // the wavelet prior: its value with weight 1, from the handle's workspace
      HIP_TRY(lmc::launch_wavelet_value(s->x[s->cur], s->C, s->prob.H, s->prob.W, s->prob.wav.p, s->prob.wav.levels, 1.f, s->prob.wav.ws, s->prob.wav.part,
                                        s->sapg_stat, st));
    else
      HIP_TRY(lmc::launch_prior_stat(s->x[s->cur], s->C, s->prob.H, s->prob.W, s->prob.prior_kind, s->sapg_stat, part, st));
    HIP_TRY(lmc::launch_sapg_update(s->sapg_stat, s->C, P, n, theta, theta_trace, gbar_trace, s->sapg_host_dev, st));
    HIP_TRY(hipEventRecord(s->sapg_ev, st));
    HIP_TRY(hipEventSynchronize(s->sapg_ev));                // the one host wait of an update
    theta = reinterpret_cast<volatile double*>(s->sapg_host)[0];
    if (!std::isfinite(theta)) return fail(LMC_E_STATE, "SAPG update %d: the prior statistic is not finite (the chains diverged)", n);
    if (n >= c.average_from) sum += theta;
    rc = lmc_sampler_set_prior_sigma(s, (float)theta);
    if (rc) return rc;
  }
  const double bar = sum / (double)(c.n_updates - c.average_from);
  theta_trace_host[0] = c.theta0;
  HIP_TRY(hipMemcpyAsync(theta_trace_host + 1, theta_trace + 1, sizeof(double) * c.n_updates, hipMemcpyDeviceToHost, st));
  if (gbar_trace_host) HIP_TRY(hipMemcpyAsync(gbar_trace_host, gbar_trace, sizeof(double) * c.n_updates, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(s->sapg_ev, st));
  HIP_TRY(hipEventSynchronize(s->sapg_ev));
  rc = lmc_sampler_set_prior_sigma(s, (float)bar);
  if (rc) return rc;
  if (theta_bar) *theta_bar = bar;
  return LMC_OK;
}
}  // namespace

extern "C" {

int lmc_prior_statistic(const lmc_problem* prob, const float* x_dev, int64_t n_img, double* stat_dev, void* stream) {
  int rc = check_stat_problem(prob);
  if (rc) return rc;
  if (!x_dev || !stat_dev || n_img < 1) return fail(LMC_E_INVALID, "bad arguments");
  if (prob->prior_kind == LMC_PRIOR_WAVELET_L1) {
    Workspace& sc = scratch_here();
    HIP_TRY(sc.wav.need(lmc::wavelet_ws_floats(n_img, prob->H, prob->W)));
    HIP_TRY(sc.wav_part.need((size_t)n_img * lmc::wavelet_partials(prob->H, prob->W, prob->tv_niter)));
    HIP_TRY(lmc::launch_wavelet_value(x_dev, n_img, prob->H, prob->W, prob->eprox_kind, prob->tv_niter, 1.f, sc.wav.p, sc.wav_part.p, stat_dev, S(stream)));
    return LMC_OK;
  }
  double* part = nullptr;
  const int nseg = lmc::prior_stat_segments(n_img, prob->H);
  if (nseg > 1) {
    Workspace& sc = scratch_here();
    HIP_TRY(sc.dbl.need((size_t)n_img * nseg));
    part = sc.dbl.p;
  }
  HIP_TRY(lmc::launch_prior_stat(x_dev, n_img, prob->H, prob->W, prob->prior_kind, stat_dev, part, S(stream)));
  return LMC_OK;
}

int lmc_sapg_dimension(const lmc_problem* prob, double* dim_eff, double* degree) {
  int rc = check_stat_problem(prob);
  if (rc) return rc;
  double d = 0.0, k = 1.0;
  sapg_dimension(prob->prior_kind, prob->H, prob->W, prob->tv_niter, &d, &k);
  if (dim_eff) *dim_eff = d;
  if (degree) *degree = k;
  return LMC_OK;
}

int lmc_sapg_update(const lmc_sapg_config* cfg, int64_t n, double theta, double gbar, double* theta_next) {
  int rc = check_sapg_config(cfg);
  if (rc) return rc;
  if (!theta_next) return fail(LMC_E_INVALID, "theta_next is NULL");
  if (!(cfg->dim_eff > 0.0)) return fail(LMC_E_INVALID, "lmc_sapg_update needs dim_eff > 0 (the default comes from lmc_sapg_dimension)");
  if (n < 0) return fail(LMC_E_INVALID, "n must be >= 0");
  if (!std::isfinite(theta) || !(theta > 0.0)) return fail(LMC_E_INVALID, "theta must be finite and > 0");
  if (!std::isfinite(gbar)) return fail(LMC_E_INVALID, "gbar must be finite");
  *theta_next = lmc::sapg_next_theta(sapg_params(*cfg, cfg->dim_eff, 1.0), (long long)n, theta, gbar);
  return LMC_OK;
}

int lmc_sampler_sapg(lmc_sampler* s, const lmc_sapg_config* cfg, const float* noise_dev, double* theta_trace_host, double* gbar_trace_host,
                     double* theta_bar, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  int rc = check_weight_settable(s);
  if (rc) return rc;
  rc = check_sapg_config(cfg);
  if (rc) return rc;
  if (!theta_trace_host) return fail(LMC_E_INVALID, "theta_trace_host is NULL");
  const int64_t iters = (int64_t)cfg->warmup_iters + (int64_t)cfg->n_updates * cfg->iters_per_update;
  if (s->noise_mode == LMC_NOISE_INJECTED && !noise_dev) return fail(LMC_E_INVALID, "noise_mode is INJECTED but noise_dev is NULL");
  if (s->noise_mode != LMC_NOISE_INJECTED && noise_dev) return fail(LMC_E_INVALID, "noise_dev given but noise_mode is not INJECTED");
  if (s->iteration + iters > 0xFFFFFFFFLL) return fail(LMC_E_STATE, "iteration counter would exceed 32 bits");
  double d = 0.0, k = 1.0;
  if (!sapg_dimension(s->prob.prior_kind, s->prob.H, s->prob.W, s->prob.wav.levels, &d, &k)) return fail(LMC_E_UNSUPPORTED, "the prior has no statistic");
  if (cfg->dim_eff > 0.0) d = cfg->dim_eff;
  if (!(d > 0.0)) return fail(LMC_E_INVALID, "the effective dimension of a %dx%d image under this prior is 0", s->prob.H, s->prob.W);
  DeviceGuard dg(s->device);
  rc = sapg_buffers(s, cfg->n_updates);
  if (rc) return rc;
  const float old = s->prob.prior_sigma;
  s->suspend_moments = true;
  rc = sapg_loop(s, *cfg, sapg_params(*cfg, d, k), noise_dev, theta_trace_host, gbar_trace_host, theta_bar, S(stream));
  s->suspend_moments = false;
  if (rc) {                       // a failed estimation leaves the weight the handle came with (the message of the failure is kept)
    const std::string msg = lmc_last_error();
    (void)lmc_sampler_set_prior_sigma(s, old);
    return fail(rc, "%s", msg.c_str());
  }
  return LMC_OK;
}

}  // extern "C"
