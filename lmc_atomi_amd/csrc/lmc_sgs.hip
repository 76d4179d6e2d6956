// The split Gibbs sampler (lmc_sgs_*; include/lmc_atomi.h holds its definition): a handle type of its own that composes existing parts.
// One iteration = the exact Gaussian draw of x | z (the spectral term: the row transforms of lmc_fft.hip around sgs_cols_gibbs_kernel, lmc_sgs_kernel.h; the
// pixel-diagonal terms: sgs_xdiag_* below), the kept iterate x into the Accumulators, then n_inner times { launch_step of the same problem without a data
// term on z, sgs_couple_kernel }.  State: x [C][H][W] and a ping-pong pair for z.
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>

#include "lmc_device.h"
#include "lmc_host.h"

using namespace lmc::host;

namespace {

constexpr unsigned kSgsMaxBlocks = 8192;   // 256 CUs x 8 workgroups of 256 threads x 4: the rest is strided over

unsigned sgs_grid(size_t units) {
  const size_t b = (units + 255) / 256;
  return (unsigned)(b < kSgsMaxBlocks ? (b ? b : 1) : kSgsMaxBlocks);
}

// The pixel-diagonal data term of a draw: b, w, m are [H][W] or NULL (w = 1, m = 1; no b: no data term at all, sf = 0)
struct SgsDiag {
  const float* b;
  const float* w;
  const float* m;
  float sf, rinv;
};

// x_p = (z_p rinv + sf w m b + sqrt(q) xi) / q,  q = sf w m^2 + rinv; IEEE sqrt and division, the products and sums as written
__device__ __forceinline__ float sgs_draw(float z, float xi, float b, float w, float m, float sf, float rinv) {
  const float cw = (sf * w) * m;
  const float q = fmaf(cw, m, rinv);
  return fmaf(z, rinv, fmaf(cw, b, sqrtf(q) * xi)) / q;
}

__device__ __forceinline__ float4 sgs_draw4(float4 z, float4 xi, float4 b, float4 w, float4 m, float sf, float rinv) {
  return make_float4(sgs_draw(z.x, xi.x, b.x, w.x, m.x, sf, rinv), sgs_draw(z.y, xi.y, b.y, w.y, m.y, sf, rinv),
                     sgs_draw(z.z, xi.z, b.z, w.z, m.z, sf, rinv), sgs_draw(z.w, xi.w, b.w, w.w, m.w, sf, rinv));
}

// The caller's field (NOISE = 1) or none (NOISE = 0: the conditional mean).  16 bytes per lane; img4 = H W / 4 (W % 4 == 0, every array 16-byte aligned)
template <int NOISE>
__global__ __launch_bounds__(256) void sgs_xdiag4_kernel(const float4* __restrict__ z, const float4* __restrict__ xi, float4* __restrict__ out, size_t n4,
                                                         size_t img4, SgsDiag D) {
  const float4 one = make_float4(1.f, 1.f, 1.f, 1.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % img4;
    const float4 b = D.b ? reinterpret_cast<const float4*>(D.b)[p] : zero;
    const float4 w = D.w ? reinterpret_cast<const float4*>(D.w)[p] : one;
    const float4 m = D.m ? reinterpret_cast<const float4*>(D.m)[p] : one;
    out[i] = sgs_draw4(z[i], NOISE ? xi[i] : zero, b, w, m, D.sf, D.rinv);
  }
}

template <int NOISE>
__global__ __launch_bounds__(256) void sgs_xdiag1_kernel(const float* __restrict__ z, const float* __restrict__ xi, float* __restrict__ out, size_t n,
                                                         size_t img, SgsDiag D) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i % img;
    out[i] = sgs_draw(z[i], NOISE ? xi[i] : 0.f, D.b ? D.b[p] : 0.f, D.w ? D.w[p] : 1.f, D.m ? D.m[p] : 1.f, D.sf, D.rinv);
  }
}

// The Philox forms draw xi with quad_normals, the counter layout of every step kernel and of launch_noise (one quad = 4 rows of one column): bit for
// bit the field lmc_sgs_noise returns.  One thread = rows 4q .. 4q+3 of columns 4g .. 4g+3 of one chain; W % 4 == 0.
__global__ __launch_bounds__(256) void sgs_xdiag_philox4_kernel(const float* __restrict__ z, float* __restrict__ out, size_t C, int H, int W, SgsDiag D,
                                                                uint32_t key0, uint32_t key1, uint32_t iteration, uint32_t chain_offset) {
  const unsigned w4 = (unsigned)W >> 2, nq = ((unsigned)H + 3u) >> 2;
  const size_t per_chain = (size_t)w4 * nq, total = per_chain * C;
  const float4 one = make_float4(1.f, 1.f, 1.f, 1.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const size_t c = u / per_chain;
    const unsigned t = (unsigned)(u - c * per_chain);
    const unsigned q = t / w4, g = t - q * w4;
    const size_t base = c * (size_t)H * W + 4u * g;
    // the loads first: in flight under the Philox arithmetic (rows past the image repeat the last row and are not stored)
    float4 zv[4], bv[4], wv[4], mv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = min(4u * q + j, (unsigned)H - 1u);
      const size_t p = (size_t)r * W + 4u * g;
      zv[j] = *reinterpret_cast<const float4*>(z + base + (size_t)r * W);
      bv[j] = D.b ? *reinterpret_cast<const float4*>(D.b + p) : zero;
      wv[j] = D.w ? *reinterpret_cast<const float4*>(D.w + p) : one;
      mv[j] = D.m ? *reinterpret_cast<const float4*>(D.m + p) : one;
    }
    float n[4][4];                                   // [column][row]
#pragma unroll
    for (int k = 0; k < 4; ++k) lmc::quad_normals(key0, key1, iteration, chain_offset + (uint32_t)c, q * (unsigned)W + 4u * g + k, n[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = 4u * q + j;
      if (r < (unsigned)H)
        *reinterpret_cast<float4*>(out + base + (size_t)r * W) =
            sgs_draw4(zv[j], make_float4(n[0][j], n[1][j], n[2][j], n[3][j]), bv[j], wv[j], mv[j], D.sf, D.rinv);
    }
  }
}

// any W: one thread = one quad (rows 4q .. 4q+3 of one column), lanes along the row
__global__ __launch_bounds__(256) void sgs_xdiag_philox1_kernel(const float* __restrict__ z, float* __restrict__ out, size_t C, int H, int W, SgsDiag D,
                                                                uint32_t key0, uint32_t key1, uint32_t iteration, uint32_t chain_offset) {
  const unsigned nq = ((unsigned)H + 3u) >> 2;
  const size_t per_chain = (size_t)nq * W, total = per_chain * C;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const size_t c = u / per_chain;
    const unsigned t = (unsigned)(u - c * per_chain);
    const unsigned q = t / (unsigned)W, col = t - q * (unsigned)W;
    const size_t base = c * (size_t)H * W + col;
    float n[4];
    lmc::quad_normals(key0, key1, iteration, chain_offset + (uint32_t)c, q * (unsigned)W + col, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = 4u * q + j;
      if (r < (unsigned)H) {
        const size_t p = (size_t)r * W + col;
        out[base + (size_t)r * W] = sgs_draw(z[base + (size_t)r * W], n[j], D.b ? D.b[p] : 0.f, D.w ? D.w[p] : 1.f, D.m ? D.m[p] : 1.f, D.sf, D.rinv);
      }
    }
  }
}

// z+ = fma(-coef, z_old - x, z'), in place in zp: 12 B read and 4 B written per pixel
__global__ __launch_bounds__(256) void sgs_couple4_kernel(float4* __restrict__ zp, const float4* __restrict__ zold, const float4* __restrict__ x, size_t n4,
                                                          float coef) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = zp[i], o = zold[i], v = x[i];
    zp[i] = make_float4(fmaf(-coef, o.x - v.x, a.x), fmaf(-coef, o.y - v.y, a.y), fmaf(-coef, o.z - v.z, a.z), fmaf(-coef, o.w - v.w, a.w));
  }
}

__global__ __launch_bounds__(256) void sgs_couple1_kernel(float* __restrict__ zp, const float* __restrict__ zold, const float* __restrict__ x, size_t n,
                                                          float coef) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) zp[i] = fmaf(-coef, zold[i] - x[i], zp[i]);
}

// out[c] = scale sum_p (x - z)^2 of chain c = blockIdx.x: the differences and squares in float64, per-thread sums over a fixed stride, then the 256
// partial sums in index order by one thread -- equal from run to run, no atomics
__global__ __launch_bounds__(256) void sgs_coupling_energy_kernel(const float* __restrict__ x, const float* __restrict__ z, size_t img, double scale,
                                                                  double* __restrict__ out) {
  __shared__ double red[256];
  const float* xc = x + (size_t)blockIdx.x * img;
  const float* zc = z + (size_t)blockIdx.x * img;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < img; i += 256) {
    const double d = (double)xc[i] - (double)zc[i];
    acc += d * d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += red[i];
    out[blockIdx.x] = scale * s;
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}

// The x-draw of a pixel-diagonal term on n_img images: noise_mode LMC_NOISE_INJECTED reads xi, LMC_NOISE_PHILOX draws it, LMC_NOISE_NONE is the mean
hipError_t launch_xdiag(const float* z, const float* xi, float* out, int64_t n_img, int H, int W, const SgsDiag& D, int noise_mode, uint32_t key0,
                        uint32_t key1, uint32_t iteration, uint32_t chain_offset, const char** name, hipStream_t st) {
  const size_t img = (size_t)H * W, n = (size_t)n_img * img;
  const bool vec = (W & 3) == 0 && aligned16({z, xi, out, D.b, D.w, D.m});
  if (noise_mode == LMC_NOISE_PHILOX) {
    const size_t nq = ((size_t)H + 3) / 4;
    if (nq * (size_t)W > 0xFFFFFFFFull) return hipErrorInvalidConfiguration;    // the quad index is one 32-bit counter word
    if (vec) {
      hipLaunchKernelGGL(sgs_xdiag_philox4_kernel, dim3(sgs_grid(nq * (size_t)(W >> 2) * (size_t)n_img)), dim3(256), 0, st, z, out, (size_t)n_img, H, W, D,
                         key0, key1, iteration, chain_offset);
    } else {
      hipLaunchKernelGGL(sgs_xdiag_philox1_kernel, dim3(sgs_grid(nq * (size_t)W * (size_t)n_img)), dim3(256), 0, st, z, out, (size_t)n_img, H, W, D, key0,
                         key1, iteration, chain_offset);
    }
    if (name) *name = vec ? "sgs_xdiag_philox4_kernel" : "sgs_xdiag_philox1_kernel";
    return hipGetLastError();
  }
  const bool inj = noise_mode == LMC_NOISE_INJECTED;
  if (inj && !xi) return hipErrorInvalidValue;
  if (vec) {
    const float4 *z4 = reinterpret_cast<const float4*>(z), *x4 = reinterpret_cast<const float4*>(xi);
    float4* o4 = reinterpret_cast<float4*>(out);
    if (inj) hipLaunchKernelGGL(sgs_xdiag4_kernel<1>, dim3(sgs_grid(n / 4)), dim3(256), 0, st, z4, x4, o4, n / 4, img / 4, D);
    else hipLaunchKernelGGL(sgs_xdiag4_kernel<0>, dim3(sgs_grid(n / 4)), dim3(256), 0, st, z4, x4, o4, n / 4, img / 4, D);
  } else {
    if (inj) hipLaunchKernelGGL(sgs_xdiag1_kernel<1>, dim3(sgs_grid(n)), dim3(256), 0, st, z, xi, out, n, img, D);
    else hipLaunchKernelGGL(sgs_xdiag1_kernel<0>, dim3(sgs_grid(n)), dim3(256), 0, st, z, xi, out, n, img, D);
  }
  if (name) *name = vec ? "sgs_xdiag4_kernel" : "sgs_xdiag1_kernel";
  return hipGetLastError();
}

hipError_t launch_couple(float* zp, const float* zold, const float* x, size_t n, float coef, hipStream_t st) {
  if ((n & 3) == 0 && aligned16({zp, zold, x})) {
    hipLaunchKernelGGL(sgs_couple4_kernel, dim3(sgs_grid(n / 4)), dim3(256), 0, st, reinterpret_cast<float4*>(zp), reinterpret_cast<const float4*>(zold),
                       reinterpret_cast<const float4*>(x), n / 4, coef);
  } else {
    hipLaunchKernelGGL(sgs_couple1_kernel, dim3(sgs_grid(n)), dim3(256), 0, st, zp, zold, x, n, coef);
  }
  return hipGetLastError();
}

// What the x-draw reads of a validated problem: the spectral tables, or the pixel-diagonal term
struct XStep {
  int spectral = 0;
  SgsDiag D{};
};

float rinv_of(float rho) { return 1.f / (rho * rho); }

// The refusals of the sampler and of lmc_sgs_xstep that concern the data term (q: the loaded problem), LMC_OK otherwise; fills X
int xstep_of(const Problem& q, float rho, const char* who, XStep& X) {
  if (q.data_kind == LMC_DATA_BLUR)
    return fail(LMC_E_UNSUPPORTED, "%s: the Hessian of a zero-padded blur is diagonal in neither the pixel nor the Fourier basis, so x | z has no closed-form draw; "
                "a periodic blur (PeriodicConvolve2D, LMC_DATA_SPECTRAL) has one", who);
  if (q.psf.on)
    return fail(LMC_E_UNSUPPORTED, "%s: the Hessian of a large PSF (zero-padded) is diagonal in neither the pixel nor the Fourier basis; a periodic blur "
                "(PeriodicConvolve2D, LMC_DATA_SPECTRAL) has a closed-form draw", who);
  if (q.radon.on)
    return fail(LMC_E_UNSUPPORTED, "%s: the Hessian of the Radon operator is diagonal in neither the pixel nor the Fourier basis, so x | z has no closed-form draw "
                "(Fourier-domain terms: FourierSampling, PeriodicConvolve2D)", who);
  if (q.sense.on)
    return fail(LMC_E_UNSUPPORTED, "%s: the Hessian of the multi-coil SENSE data term (LMC_DATA_SENSE) is diagonal in neither the pixel nor the Fourier basis, so "
                "x | z has no closed-form draw; use MYULA or SK-ROCK", who);
  if (q.term == lmc::kTermPois) return fail(LMC_E_UNSUPPORTED, "%s: with the Poisson data term the conditional x | z is not Gaussian", who);
  if (q.term == lmc::kTermHub) return fail(LMC_E_UNSUPPORTED, "%s: with the Huber data term the conditional x | z is not Gaussian", who);
  if (q.ncvx_kind != LMC_NCVX_NONE) return fail(LMC_E_UNSUPPORTED, "%s: the non-convex terms are not built for it: ncvx_kind must be LMC_NCVX_NONE", who);
  X.D.rinv = rinv_of(rho);
  X.D.sf = q.data_kind == LMC_DATA_NONE ? 0.f : q.sigma_f;
  if (q.fft.on) { X.spectral = 1; return LMC_OK; }
  const size_t img = (size_t)q.H * q.W;
  if (q.data_kind != LMC_DATA_NONE) X.D.b = q.y;
  if (q.data_kind == LMC_DATA_MASK) X.D.m = q.mask;
  if (q.term == lmc::kTermWl2) X.D.w = q.y + img;      // y = [2][H][W]: observation, weights
  return LMC_OK;
}

// x = the draw of x | z on n images.  Spectral: F bound to a spectrum buffer of 2 n images (the second half takes the noise spectrum); xi: the white field
// or NULL.  Pixel-diagonal: launch_xdiag.
int run_xstep(const XStep& X, const Problem& q, const float* z, const float* xi, float* out, int64_t n, int noise_mode, uint32_t key0, uint32_t key1,
              uint32_t iteration, uint32_t chain_offset, const char** name, hipStream_t st) {
  if (!X.spectral) {
    HIP_TRY(launch_xdiag(z, xi, out, n, q.H, q.W, X.D, noise_mode, key0, key1, iteration, chain_offset, name, st));
    return LMC_OK;
  }
  const lmc::FftOp& F = q.fft;
  float2* nspec = nullptr;
  if (noise_mode == LMC_NOISE_PHILOX) {      // the field into `out` (overwritten by the last launch), its row transform from there
    HIP_TRY(lmc::launch_noise(out, (int)n, q.H, q.W, key0, key1, iteration, chain_offset, st));
    xi = out;
  }
  if (noise_mode != LMC_NOISE_NONE) {
    nspec = F.spec + (size_t)n * q.H * (q.W / 2 + 1);
    HIP_TRY(lmc::launch_fft_rows_fwd(xi, nspec, F.tw, n, q.H, q.W, st));
  }
  HIP_TRY(lmc::launch_fft_rows_fwd(z, F.spec, F.tw, n, q.H, q.W, st));
  HIP_TRY(lmc::launch_fft_gibbs(F.spec, nspec, F.tab, F.tw, n, q.H, q.W, X.D.rinv, X.D.sf, st));
  HIP_TRY(lmc::launch_fft_rows_inv(lmc::kFftStore, F.spec, out, nullptr, F.tw, n, q.H, q.W, 0.f, 0.f, st));
  if (name) *name = "sgs_cols_gibbs_kernel";
  return LMC_OK;
}

bool positive_finite(float v) { return std::isfinite(v) && v > 0.f; }

}  // namespace

struct lmc_sgs {
  int device = -1;
  int C = 0, H = 0, W = 0;
  int64_t chain_offset = 0;
  float rho = 0, tau = 0, gamma = 0, epsg = 1;
  int n_inner = 1;
  uint64_t seed = 0;
  int noise_mode = 0;
  int moments = 0, burn_in = 0, thin = 1;
  int64_t iteration = 0;
  Problem prob;                 // the whole problem: its data term feeds the x-draw and f, its prior the z-step (a launch without a data term) and g
  XStep xs;
  lmc::StepArgs base{};         // the z-step without its coupling: (1 - tau / gamma) z + (tau / gamma) prox + sqrt(2 tau) xi_z, the Philox key of plane 1
  Accumulators acc;
  Workspace ws;
  Owned own;
  float* x = nullptr;
  float* z[2] = {nullptr, nullptr};
  int cur = 0;
  std::string kernel_name;

  size_t block() const { return (size_t)C * H * W; }
  uint32_t key0() const { return (uint32_t)(seed & 0xFFFFFFFFu); }
  uint32_t key1(int plane) const { return (uint32_t)(seed >> 32) + (uint32_t)plane; }      // plane p: the seed (seed + (p << 32)) mod 2^64
};

namespace {

void destroy(lmc_sgs* s) {
  s->own.release();
  s->ws.release();
  s->acc.release();
  delete s;
}

int alloc_failed(lmc_sgs* s, hipError_t e) {
  const int rc = fail(e == hipErrorOutOfMemory ? LMC_E_NOMEM : LMC_E_HIP, "sampler allocation failed: %s", hipGetErrorString(e));
  destroy(s);
  return rc;
}

bool kept(const lmc_sgs* s, int64_t it) { return s->moments && it >= s->burn_in && (it - s->burn_in) % s->thin == 0; }

// what both entry points refuse of the raw problem before it is loaded
int check_raw_problem(const lmc_problem* p, const char* who) {
  if (!p) return fail(LMC_E_INVALID, "lmc_problem is NULL");
  if (p->struct_size != sizeof(lmc_problem))
    return fail(LMC_E_INVALID, "lmc_problem.struct_size %u != %zu (ABI mismatch)", p->struct_size, sizeof(lmc_problem));
  if (p->prior_kind == LMC_PRIOR_VTV)
    return fail(LMC_E_UNSUPPORTED, "%s: LMC_PRIOR_VTV acts on multi-channel images (lmc_mch_create); a multi-channel split Gibbs sampler is not built", who);
  if (p->data_kind == LMC_DATA_SPECTRAL && !lmc::fft_shape_ok(p->H, p->W))
    return fail(LMC_E_INVALID, "%s: the spectral x-draw takes sides that are powers of two in %d .. %d (got %dx%d)", who, lmc::kFftMin, lmc::kFftMax, p->H, p->W);
  return LMC_OK;
}

}  // namespace

namespace lmc::host {

// lmc_sgs_xstep behind its entry point (lmc_capi.hip): sc is the workspace the spectrum buffers are taken from
int sgs_xstep(const lmc_problem* prob, const float* z_dev, const float* noise_dev, float* out_dev, int64_t n_img, float rho, Workspace& sc, hipStream_t st) {
  static const char* const who = "lmc_sgs_xstep";
  int rc = check_raw_problem(prob, who);
  if (rc) return rc;
  if (!z_dev || !out_dev || z_dev == out_dev || noise_dev == out_dev) return fail(LMC_E_INVALID, "bad pointers (in-place not allowed)");
  if (n_img < 1 || n_img > (1 << 24)) return fail(LMC_E_INVALID, "bad n_img %lld", (long long)n_img);
  if (!positive_finite(rho) || !positive_finite(rinv_of(rho))) return fail(LMC_E_INVALID, "rho must be finite and > 0 (got %g)", (double)rho);
  Problem q;
  rc = load_problem(prob, q);
  XStep xs;
  if (!rc) rc = xstep_of(q, rho, who, xs);
  if (rc) return rc;
  if (q.fft.on) HIP_TRY(sc.bind_fft(q.fft, 2 * lmc::fft_spec_floats(n_img, q.H, q.W), 0));
  return run_xstep(xs, q, z_dev, noise_dev, out_dev, n_img, noise_dev ? LMC_NOISE_INJECTED : LMC_NOISE_NONE, 0, 0, 0, 0, nullptr, st);
}

}  // namespace lmc::host

extern "C" {

int lmc_sgs_create(const lmc_sgs_config* cfg, lmc_sgs** out) {
  static const char* const who = "lmc_sgs_create";
  if (!cfg || !out) return fail(LMC_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(lmc_sgs_config))
    return fail(LMC_E_INVALID, "lmc_sgs_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size, sizeof(lmc_sgs_config));
  if (cfg->n_chains < 1 || cfg->n_chains > (1 << 24)) return fail(LMC_E_INVALID, "n_chains must be in 1 .. 2^24");
  if (cfg->chain_offset < 0 || cfg->chain_offset + cfg->n_chains > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "global chain ids must fit 32 bits");
  if (!positive_finite(cfg->rho) || !positive_finite(cfg->tau) || !positive_finite(cfg->gamma))
    return fail(LMC_E_INVALID, "rho, tau and gamma must be finite and > 0 (got %g, %g, %g)", (double)cfg->rho, (double)cfg->tau, (double)cfg->gamma);
  if (!positive_finite(rinv_of(cfg->rho))) return fail(LMC_E_INVALID, "1 / rho^2 is not finite and > 0 in float32 (rho = %g)", (double)cfg->rho);
  if (!(cfg->epsg >= 0.f)) return fail(LMC_E_INVALID, "epsg must be >= 0");
  if (cfg->n_inner < 1 || cfg->n_inner > LMC_MAX_SGS_INNER) return fail(LMC_E_INVALID, "n_inner %d outside 1..%d", cfg->n_inner, LMC_MAX_SGS_INNER);
  if (cfg->noise_mode < LMC_NOISE_PHILOX || cfg->noise_mode > LMC_NOISE_NONE) return fail(LMC_E_INVALID, "bad noise_mode");
  if (cfg->moments && cfg->thin < 1) return fail(LMC_E_INVALID, "thin must be >= 1");
  if (cfg->moments && cfg->burn_in < 0) return fail(LMC_E_INVALID, "burn_in must be >= 0");
  const lmc_problem* p = &cfg->problem;
  int rc = check_raw_problem(p, who);
  if (rc) return rc;
  if (p->tv_rtol > 0.f) return fail(LMC_E_UNSUPPORTED, "%s: tv_rtol > 0 (early exit of the prox) is not built for it: use the fixed count, tv_rtol = 0", who);
  if (p->tv_warm) return fail(LMC_E_UNSUPPORTED, "%s: tv_warm (warm-started dual) is not built for it", who);
  if (p->prox_scale) return fail(LMC_E_UNSUPPORTED, "%s: prox_scale (array-valued epsg) belongs to the MYULA sampler", who);
  lmc_sgs* s = new (std::nothrow) lmc_sgs();
  if (!s) return fail(LMC_E_NOMEM, "host allocation failed");
  Problem& q = s->prob;
  rc = load_problem(p, q);
  if (!rc) rc = xstep_of(q, cfg->rho, who, s->xs);
  if (rc) { delete s; return rc; }
  if (hipGetDevice(&s->device) != hipSuccess) { delete s; return fail(LMC_E_HIP, "hipGetDevice failed"); }
  s->C = cfg->n_chains; s->H = q.H; s->W = q.W;
  s->chain_offset = cfg->chain_offset;
  s->rho = cfg->rho; s->tau = cfg->tau; s->gamma = cfg->gamma; s->epsg = cfg->epsg;
  s->n_inner = cfg->n_inner;
  s->seed = cfg->seed;
  s->noise_mode = cfg->noise_mode;
  s->moments = cfg->moments; s->burn_in = cfg->burn_in; s->thin = cfg->thin < 1 ? 1 : cfg->thin;
  // the z-step: t = 0, so the launch carries no data term whatever the problem's is
  const float b = s->tau / s->gamma;
  {
    Problem zq = q;      // what the step launch sees: the prior alone (the rules of the data terms' own step kernels do not apply to it)
    zq.data_kind = LMC_DATA_NONE; zq.term = lmc::kTermL2; zq.fft.on = 0;
    rc = check_step_problem(zq, b);
  }
  if (!rc) rc = make_step_args(q, 1.f - b, 0.f, b, s->epsg * s->gamma, std::sqrt(2.f * s->tau), s->base);
  if (rc) { delete s; return rc; }
  lmc::StepArgs& A = s->base;
  A.C = s->C;
  A.noise_mode = s->noise_mode;
  A.key0 = s->key0();
  A.key1 = s->key1(1);
  A.chain_offset = (uint32_t)s->chain_offset;
  const size_t n = s->block();
  hipError_t e = s->own.alloc(&s->x, n, true);
  if (e == hipSuccess) e = s->own.alloc(&s->z[0], n, true);
  if (e == hipSuccess) e = s->own.alloc(&s->z[1], n, false);
  // every work buffer of the z-step and of the energies here and never inside lmc_sgs_step; the spectrum buffer twice: z and the noise
  if (e == hipSuccess) e = prepare(s->ws, q, A, s->C, s->epsg * s->gamma, kForStep | kForEnergies, nullptr);
  if (e == hipSuccess && q.fft.on)
    e = s->ws.bind_fft(q.fft, 2 * lmc::fft_spec_floats(s->C, q.H, q.W), lmc::fft_value_partials(s->C, q.H, q.W));
  if (e == hipSuccess && s->moments) e = s->acc.alloc(s->C, s->chain_offset, s->H, s->W);
  if (e != hipSuccess) return alloc_failed(s, e);
  s->kernel_name = "(no step launched yet)";
  *out = s;
  return LMC_OK;
}

void lmc_sgs_destroy(lmc_sgs* s) {
  if (!s) return;
  DeviceGuard dg(s->device);
  destroy(s);
}

int lmc_sgs_set_state(lmc_sgs* s, const float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  const size_t n = s->block();
  HIP_TRY(hipMemcpyAsync(s->x, x_dev, sizeof(float) * n, hipMemcpyDeviceToDevice, S(stream)));
  HIP_TRY(hipMemcpyAsync(s->z[s->cur], x_dev + n, sizeof(float) * n, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_sgs_get_state(lmc_sgs* s, float* x_dev, void* stream) {
  if (!s || !x_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  const size_t n = s->block();
  HIP_TRY(hipMemcpyAsync(x_dev, s->x, sizeof(float) * n, hipMemcpyDeviceToDevice, S(stream)));
  HIP_TRY(hipMemcpyAsync(x_dev + n, s->z[s->cur], sizeof(float) * n, hipMemcpyDeviceToDevice, S(stream)));
  return LMC_OK;
}

int lmc_sgs_step(lmc_sgs* s, int32_t n_iters, const float* noise_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (n_iters < 0) return fail(LMC_E_INVALID, "n_iters < 0");
  if (s->noise_mode == LMC_NOISE_INJECTED && !noise_dev && n_iters > 0) return fail(LMC_E_INVALID, "noise_mode is INJECTED but noise_dev is NULL");
  if (s->noise_mode != LMC_NOISE_INJECTED && noise_dev) return fail(LMC_E_INVALID, "noise_dev given but noise_mode is not INJECTED");
  if ((s->iteration + n_iters) * s->n_inner > 0xFFFFFFFFLL) return fail(LMC_E_STATE, "iteration counter times n_inner would exceed 32 bits");
  hipStream_t st = S(stream);
  const size_t blk = s->block(), per_iter = (size_t)(1 + s->n_inner) * blk;
  const float coef = s->tau * s->xs.D.rinv;
  for (int k = 0; k < n_iters; ++k) {
    const float* nz = noise_dev ? noise_dev + (size_t)k * per_iter : nullptr;
    // 1. x | z, exact
    const char* xname = nullptr;
    int rc = run_xstep(s->xs, s->prob, s->z[s->cur], nz, s->x, s->C, s->noise_mode, s->key0(), s->key1(0), (uint32_t)s->iteration,
                       (uint32_t)s->chain_offset, &xname, st);
    if (rc) return rc;
    if (kept(s, s->iteration)) {
      HIP_TRY(s->acc.reduce(s->x, st));
      s->acc.count += (uint64_t)s->C;
    }
    // 2. z | x: the step of the problem without a data term, then the coupling with the z it started from
    const char* kname = nullptr;
    for (int j = 0; j < s->n_inner; ++j) {
      lmc::StepArgs A = s->base;
      A.x_in = s->z[s->cur];
      A.x_out = s->z[s->cur ^ 1];
      A.iteration = (uint32_t)(s->iteration * s->n_inner + j);
      A.noise = nz ? nz + (size_t)(1 + j) * blk : nullptr;
      sanitize_pointers(A);
      hipError_t e = launch_step(A, s->prob, s->ws, st, &kname);
      if (e == hipErrorInvalidConfiguration) return fail(LMC_E_UNSUPPORTED, "no step-kernel variant covers this configuration");
      HIP_TRY(e);
      HIP_TRY(launch_couple(s->z[s->cur ^ 1], s->z[s->cur], s->x, blk, coef, st));
      s->cur ^= 1;
    }
    if (xname && kname) s->kernel_name = std::string(xname) + " + " + kname + " + sgs_couple_kernel";
    ++s->iteration;
  }
  return LMC_OK;
}

int64_t lmc_sgs_iteration(const lmc_sgs* s) { return s ? s->iteration : -1; }

int lmc_sgs_set_iteration(lmc_sgs* s, int64_t it) {
  if (!s || it < 0 || it > 0xFFFFFFFFLL || it * s->n_inner > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  s->iteration = it;
  return LMC_OK;
}

int lmc_sgs_get_moments(lmc_sgs* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_get_moments(s->acc, s->moments, sum_dev, sumsq_dev, count, S(stream));
}

int lmc_sgs_reset_moments(lmc_sgs* s, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  if (!s->moments) return fail(LMC_E_STATE, "sampler was created with moments = 0");
  return s->acc.reset(S(stream));
}

int lmc_sgs_set_chain_groups(lmc_sgs* s, int32_t n_groups) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_set_chain_groups(s->acc, s->moments, n_groups);
}

int lmc_sgs_get_group_moments(lmc_sgs* s, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  return accum_get_group_moments(s->acc, sum_dev, sumsq_dev, counts_host, S(stream));
}

int lmc_sgs_energies(lmc_sgs* s, double* f_out_dev, double* g_out_dev, double* coupling_out_dev, void* stream) {
  if (!s) return fail(LMC_E_INVALID, "NULL sampler");
  DeviceGuard dg(s->device);
  hipStream_t st = S(stream);
  if (f_out_dev) {
    const int rc = problem_energies(s->prob, s->x, s->C, f_out_dev, nullptr, s->ws, st);
    if (rc) return rc;
  }
  if (g_out_dev) {
    const int rc = problem_energies(s->prob, s->z[s->cur], s->C, nullptr, g_out_dev, s->ws, st);
    if (rc) return rc;
  }
  if (coupling_out_dev) {
    hipLaunchKernelGGL(sgs_coupling_energy_kernel, dim3((unsigned)s->C), dim3(256), 0, st, s->x, s->z[s->cur], (size_t)s->H * s->W,
                       0.5 / ((double)s->rho * (double)s->rho), coupling_out_dev);
    HIP_TRY(hipGetLastError());
  }
  return LMC_OK;
}

int lmc_sgs_noise(lmc_sgs* s, int64_t iteration, int32_t plane_and_inner, float* out_dev, void* stream) {
  if (!s || !out_dev) return fail(LMC_E_INVALID, "NULL argument");
  DeviceGuard dg(s->device);
  if (plane_and_inner < 0 || plane_and_inner > s->n_inner) return fail(LMC_E_INVALID, "plane_and_inner %d outside 0..n_inner = %d", plane_and_inner, s->n_inner);
  if (iteration < 0 || (iteration + 1) * s->n_inner - 1 > 0xFFFFFFFFLL) return fail(LMC_E_INVALID, "bad iteration");
  const int plane = plane_and_inner ? 1 : 0;
  const int64_t counter = plane ? iteration * s->n_inner + (plane_and_inner - 1) : iteration;
  HIP_TRY(lmc::launch_noise(out_dev, s->C, s->H, s->W, s->key0(), s->key1(plane), (uint32_t)counter, (uint32_t)s->chain_offset, S(stream)));
  return LMC_OK;
}

const char* lmc_sgs_kernel_name(const lmc_sgs* s) { return s ? s->kernel_name.c_str() : ""; }

}  // extern "C"
