// SK-ROCK stage 1 (include/lmc_atomi.h, lmc_skrock_create): the perturbed point Y = X + nu_1 sqrt(2 delta) Z the first drift evaluation runs on.
// Every other stage of the scheme is a launch of the fused step kernel; this is the one pass of its own: streaming, 4 B read + 4 B written per
// chain-pixel, the Philox arithmetic of the field under the loads.
//   Philox form    Z is drawn in place with quad_normals, the counter layout of every step kernel (ctr = (quad, iteration, global chain, stream
//                  tag), key = seed; one quad = 4 rows of one column): bit for bit the field the step launch that follows draws again.
//   injected form  Z is the caller's array.
// 16 bytes per lane where the rows allow it (W % 4 == 0: one thread = a 4 x 4 block = four quads, a wave = 1 KiB of each of its four rows), a
// plain form (one thread = one quad) for any W.  The grid is one-dimensional and capped, the (chain, quad) units are strided over: any chain count.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

namespace {
constexpr unsigned kPerturbMaxBlocks = 8192;   // 256 CUs x 8 workgroups of 256 threads x 4: the rest is strided over

unsigned perturb_grid(size_t units) {
  const size_t b = (units + 255) / 256;
  return (unsigned)(b < kPerturbMaxBlocks ? (b ? b : 1) : kPerturbMaxBlocks);
}
}  // namespace

// one thread = rows 4q .. 4q+3 of columns 4g .. 4g+3 of one chain; W % 4 == 0
__global__ __launch_bounds__(256) void skrock_perturb_philox4_kernel(const float* __restrict__ x, float* __restrict__ out, size_t C, int H, int W,
                                                                     float coef, uint32_t key0, uint32_t key1, uint32_t iteration,
                                                                     uint32_t chain_offset) {
  const unsigned w4 = (unsigned)W >> 2, nq = ((unsigned)H + 3u) >> 2;
  const size_t per_chain = (size_t)w4 * nq, total = per_chain * C;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const size_t c = u / per_chain;
    const unsigned t = (unsigned)(u - c * per_chain);
    const unsigned q = t / w4, g = t - q * w4;
    const size_t base = c * (size_t)H * W + 4u * g;
    // the loads first: in flight under the Philox arithmetic (rows past the image repeat the last row and are not stored)
    float4 xv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = min(4u * q + j, (unsigned)H - 1u);
      xv[j] = *reinterpret_cast<const float4*>(x + base + (size_t)r * W);
    }
    float n[4][4];                                   // [column][row]
#pragma unroll
    for (int k = 0; k < 4; ++k) quad_normals(key0, key1, iteration, chain_offset + (uint32_t)c, q * (unsigned)W + 4u * g + k, n[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = 4u * q + j;
      if (r < (unsigned)H)
        *reinterpret_cast<float4*>(out + base + (size_t)r * W) =
            make_float4(fmaf(coef, n[0][j], xv[j].x), fmaf(coef, n[1][j], xv[j].y), fmaf(coef, n[2][j], xv[j].z), fmaf(coef, n[3][j], xv[j].w));
    }
  }
}

// any W: one thread = one quad (rows 4q .. 4q+3 of one column), lanes along the row
__global__ __launch_bounds__(256) void skrock_perturb_philox1_kernel(const float* __restrict__ x, float* __restrict__ out, size_t C, int H, int W,
                                                                     float coef, uint32_t key0, uint32_t key1, uint32_t iteration,
                                                                     uint32_t chain_offset) {
  const unsigned nq = ((unsigned)H + 3u) >> 2;
  const size_t per_chain = (size_t)nq * W, total = per_chain * C;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const size_t c = u / per_chain;
    const unsigned t = (unsigned)(u - c * per_chain);
    const unsigned q = t / (unsigned)W, col = t - q * (unsigned)W;
    const size_t base = c * (size_t)H * W + col;
    float xv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] = x[base + (size_t)min(4u * q + j, (unsigned)H - 1u) * W];
    float n[4];
    quad_normals(key0, key1, iteration, chain_offset + (uint32_t)c, q * (unsigned)W + col, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = 4u * q + j;
      if (r < (unsigned)H) out[base + (size_t)r * W] = fmaf(coef, n[j], xv[j]);
    }
  }
}

__global__ __launch_bounds__(256) void skrock_perturb4_kernel(const float4* __restrict__ x, const float4* __restrict__ xi, float4* __restrict__ out,
                                                              size_t n4, float coef) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = x[i], z = xi[i];
    out[i] = make_float4(fmaf(coef, z.x, a.x), fmaf(coef, z.y, a.y), fmaf(coef, z.z, a.z), fmaf(coef, z.w, a.w));
  }
}

__global__ __launch_bounds__(256) void skrock_perturb1_kernel(const float* __restrict__ x, const float* __restrict__ xi, float* __restrict__ out,
                                                              size_t n, float coef) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = fmaf(coef, xi[i], x[i]);
}

hipError_t launch_skrock_perturb_philox(const float* x, float* out, int64_t C, int H, int W, float coef, uint32_t key0, uint32_t key1,
                                        uint32_t iteration, uint32_t chain_offset, hipStream_t st) {
  if (C < 1 || H < 1 || W < 1) return hipErrorInvalidValue;
  const size_t nq = ((size_t)H + 3) / 4;
  if (nq * (size_t)W > 0xFFFFFFFFull) return hipErrorInvalidConfiguration;    // the quad index is one 32-bit counter word
  const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (vec) {
    hipLaunchKernelGGL(skrock_perturb_philox4_kernel, dim3(perturb_grid(nq * (size_t)(W >> 2) * (size_t)C)), dim3(256), 0, st, x, out, (size_t)C, H, W,
                       coef, key0, key1, iteration, chain_offset);
  } else {
    hipLaunchKernelGGL(skrock_perturb_philox1_kernel, dim3(perturb_grid(nq * (size_t)W * (size_t)C)), dim3(256), 0, st, x, out, (size_t)C, H, W, coef,
                       key0, key1, iteration, chain_offset);
  }
  return hipGetLastError();
}

hipError_t launch_skrock_perturb(const float* x, const float* xi, float* out, size_t n, float coef, hipStream_t st) {
  if (n == 0) return hipErrorInvalidValue;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(out);
  if ((n & 3) == 0 && (bits & 15) == 0) {
    hipLaunchKernelGGL(skrock_perturb4_kernel, dim3(perturb_grid(n / 4)), dim3(256), 0, st, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(xi), reinterpret_cast<float4*>(out), n / 4, coef);
  } else {
    hipLaunchKernelGGL(skrock_perturb1_kernel, dim3(perturb_grid(n)), dim3(256), 0, st, x, xi, out, n, coef);
  }
  return hipGetLastError();
}

}  // namespace lmc
