// Chain-group moments (include/lmc_atomi.h, lmc_sampler_set_chain_groups): one pass over a kept iterate x[C][H][W] that ADDS into A[G][H][W] and
// B[G][H][W] (float64) the sums of x and of x^2 over the chains of every group; chain c belongs to group (chain_offset + c) mod G.  The fp32
// sample is widened first, so its square is exact in float64 and A, B carry only the rounding of float64 sums.
//
// One owner per (group, pixel) and launch: a thread owns one group and 4 consecutive pixels of the flattened image, walks the chains of its group
// in ascending order with 16-byte loads (a wave = 1 KiB of one chain per load, four loads in flight), keeps its 8 float64 sums in registers
// and finishes with ONE plain read-add-write of its 64 bytes of A and B.  No float atomics: two runs give equal bits, and launches on one stream
// are ordered, which is all the accumulators ask of their callers.  A scalar form (one thread = one group and one pixel) takes the images whose
// size is no multiple of 4 and the arrays that are not 16-byte aligned.  The grid is one-dimensional and capped, the (group, pixel-quad) units
// are strided over: any chain count, any image size.  No LDS, no scratch: on the side stream the pass shares a compute unit with the pipe
// kernel, whose LDS is full.
//
// Bytes per kept iterate: 4 C HW read of x, plus 32 G HW of accumulator traffic (A and B, 8 bytes each, read and written once).  At G = 64 and
// C = 1024 that is 2048 HW on top of 4096 HW: half as much again as the read of x, which is the read the moment reduction makes as well.
// Parallelism is G HW / 4 threads whatever C is, each walking C / G chains serially: sized for images (512 x 512: 0.5 M threads at G = 8); a tiny
// image with very many chains runs on a handful of threads and is bound by load latency -- correct, not the use case.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

namespace {
constexpr unsigned kGroupMaxBlocks = 8192;   // 256 CUs x 8 workgroups of 256 threads x 4: the rest is strided over

unsigned group_grid(size_t units) {
  const size_t b = (units + 255) / 256;
  return (unsigned)(b < kGroupMaxBlocks ? (b ? b : 1) : kGroupMaxBlocks);
}

__device__ __forceinline__ void group_add4(const float4 v, double (&a)[4], double (&b)[4]) {
  const double d0 = (double)v.x, d1 = (double)v.y, d2 = (double)v.z, d3 = (double)v.w;
  a[0] += d0; a[1] += d1; a[2] += d2; a[3] += d3;
  b[0] += d0 * d0; b[1] += d1 * d1; b[2] += d2 * d2; b[3] += d3 * d3;      // d * d is exact: fused or not, one rounding
}
}  // namespace

// one thread = group g, pixels 4q .. 4q+3; img % 4 == 0, x / A / B 16-byte aligned.  first = chain_offset mod G: local chain c has group
// (first + c) mod G, so group g starts at local chain (g - first) mod G and takes every G-th chain from there.
__global__ __launch_bounds__(256) void group_moments4_kernel(const float* __restrict__ x, size_t C, unsigned first, size_t img, unsigned G,
                                                             double* __restrict__ A, double* __restrict__ B) {
  const size_t nq = img >> 2, total = nq * G;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const unsigned g = (unsigned)(u / nq);
    const size_t p = (u - (size_t)g * nq) << 2;
    double a[4] = {0., 0., 0., 0.}, b[4] = {0., 0., 0., 0.};
    size_t c = (g + G - first) % G;
    for (; c + 3 * (size_t)G < C; c += 4 * (size_t)G) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(x + (c + (size_t)j * G) * img + p);
#pragma unroll
      for (int j = 0; j < 4; ++j) group_add4(v[j], a, b);
    }
    for (; c < C; c += G) group_add4(*reinterpret_cast<const float4*>(x + c * img + p), a, b);
    double2* pa = reinterpret_cast<double2*>(A + (size_t)g * img + p);
    double2* pb = reinterpret_cast<double2*>(B + (size_t)g * img + p);
    const double2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
    pa[0] = make_double2(a0.x + a[0], a0.y + a[1]);
    pa[1] = make_double2(a1.x + a[2], a1.y + a[3]);
    pb[0] = make_double2(b0.x + b[0], b0.y + b[1]);
    pb[1] = make_double2(b1.x + b[2], b1.y + b[3]);
  }
}

// any image size and alignment: one thread = group g, pixel p
__global__ __launch_bounds__(256) void group_moments1_kernel(const float* __restrict__ x, size_t C, unsigned first, size_t img, unsigned G,
                                                             double* __restrict__ A, double* __restrict__ B) {
  const size_t total = img * G;
  for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (size_t)gridDim.x * blockDim.x) {
    const unsigned g = (unsigned)(u / img);
    const size_t p = u - (size_t)g * img;
    double a = 0., b = 0.;
    size_t c = (g + G - first) % G;
    for (; c + 3 * (size_t)G < C; c += 4 * (size_t)G) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = x[(c + (size_t)j * G) * img + p];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)v[j];
        a += d;
        b += d * d;
      }
    }
    for (; c < C; c += G) {
      const double d = (double)x[c * img + p];
      a += d;
      b += d * d;
    }
    A[u] += a;
    B[u] += b;
  }
}

// A[G][H][W] += sum x, B[G][H][W] += sum x^2 over the chains of every group of x[C][H][W].  2 <= G <= LMC_MAX_CHAIN_GROUPS (the caller checks).
hipError_t launch_group_moments(const float* x, int64_t C, int64_t chain_offset, int H, int W, int G, double* A, double* B, hipStream_t st) {
  if (C < 1 || H < 1 || W < 1 || G < 1) return hipErrorInvalidValue;
  const size_t img = (size_t)H * W;
  const unsigned first = (unsigned)(((chain_offset % G) + G) % G);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B);
  if ((img & 3) == 0 && (bits & 15) == 0) {
    hipLaunchKernelGGL(group_moments4_kernel, dim3(group_grid((img >> 2) * (size_t)G)), dim3(256), 0, st, x, (size_t)C, first, img, (unsigned)G, A, B);
  } else {
    hipLaunchKernelGGL(group_moments1_kernel, dim3(group_grid(img * (size_t)G)), dim3(256), 0, st, x, (size_t)C, first, img, (unsigned)G, A, B);
  }
  return hipGetLastError();
}

}  // namespace lmc
