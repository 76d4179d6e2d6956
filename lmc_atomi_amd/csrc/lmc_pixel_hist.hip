// Pixel-wise posterior histograms: one pass over a kept iterate x[C][H][W] that ADDS into counts[B + 2][H][W] (unsigned 64-bit).  For a
// sample v at pixel p, in fp32, t = (v - lo[p]) * scale[p] (one subtraction, then one multiplication):
//   row 0          t < 0
//   row 1 + floor(t)   0 <= t < B
//   row B + 1      everything else (t >= B, +inf, NaN)
// so the rows of a pixel sum to the number of samples.  Integer atomics: the result does not depend on the launch shape or on their order.
//
// The counters of a pixel live in registers, bit-sliced: the (up to 64) rows of a pixel are the bits of a 64-bit one-hot word 1 << row, and
// bit r of plane k is bit k of the count of row r.  Eight chains are added at a time with seven carry-save adders (planes 0 .. 2 are the
// running ones, twos and fours; the carry out of the fours ripples through the planes above), the chains left over one by one.  A launch
// segment is at most kHistSeg <= 2047 chains, so eleven planes hold every count; the flush walks the set bits of the OR of the planes, one
// atomicAdd per non-empty row and segment.  The atomics, not the read of x, are what the pass costs -- its time grows with the number of
// segments (measured: DESIGN 3.3) -- hence segments as long as the planes allow.  No LDS, no scratch, every register index is static.
#include <cstdlib>

#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kHistSeg = 2040;    // chains per segment at most: a multiple of 8 below 2^kHistPlanes
constexpr int kHistPlanes = 11;
typedef unsigned long long hist_word;
static_assert(kHistSeg % 8 == 0 && kHistSeg < (1 << kHistPlanes), "a segment's count of one row must fit the planes");

__device__ __forceinline__ hist_word hist_onehot(float v, float lo, float scale, int B, float fB) {
  const float t = __fmul_rn(__fsub_rn(v, lo), scale);
  const int r = t < 0.f ? 0 : (t < fB ? 1 + (int)t : B + 1);     // NaN fails both comparisons
  return (hist_word)1 << r;
}

// a + b + c = sum + 2 carry, bit by bit; the sum replaces a
__device__ __forceinline__ hist_word hist_csa(hist_word& a, hist_word b, hist_word c) {
  const hist_word u = a ^ b;
  const hist_word carry = (a & b) | (u & c);
  a = u ^ c;
  return carry;
}

template <int FROM>
__device__ __forceinline__ void hist_ripple(hist_word (&P)[kHistPlanes], hist_word carry) {
#pragma unroll
  for (int k = FROM; k < kHistPlanes; ++k) {
    const hist_word t = P[k] & carry;
    P[k] ^= carry;
    carry = t;
  }
}

__device__ __forceinline__ void hist_add8(hist_word (&P)[kHistPlanes], const hist_word (&w)[8]) {
  const hist_word a2 = hist_csa(P[0], w[0], w[1]);
  const hist_word b2 = hist_csa(P[0], w[2], w[3]);
  const hist_word a4 = hist_csa(P[1], a2, b2);
  const hist_word c2 = hist_csa(P[0], w[4], w[5]);
  const hist_word d2 = hist_csa(P[0], w[6], w[7]);
  const hist_word b4 = hist_csa(P[1], c2, d2);
  hist_ripple<3>(P, hist_csa(P[2], a4, b4));
}

__device__ __forceinline__ void hist_flush(const hist_word (&P)[kHistPlanes], hist_word* __restrict__ counts, size_t img, size_t p) {
  hist_word m = 0;
#pragma unroll
  for (int k = 0; k < kHistPlanes; ++k) m |= P[k];
  while (m) {
    const int r = __ffsll((long long)m) - 1;
    hist_word n = 0;
#pragma unroll
    for (int k = 0; k < kHistPlanes; ++k) n |= ((P[k] >> r) & 1ull) << k;
    atomicAdd(&counts[(size_t)r * img + p], n);
    m &= m - 1;
  }
}

constexpr int kHistPix = 2;       // pixels per lane

// A wave owns 128 consecutive pixels; lane l holds pixels l and 64 + l of them, so that a wave's loads of one chain are two
// runs of 256 contiguous bytes and -- what decides the speed -- its 64 atomics of one pixel slot and row cover 512 contiguous bytes (eight
// cache lines) of that row of counts.  Any image size: a slot past the image reads pixel 0 and is never flushed.  blockIdx.y = chain segment
// of seg_len <= kHistSeg chains.
__global__ __launch_bounds__(256) void pixel_hist_kernel(const float* __restrict__ x, int C, size_t img, int seg_len, int B,
                                                         const float* __restrict__ lo, const float* __restrict__ scale,
                                                         hist_word* __restrict__ counts) {
  const size_t p0 = ((size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63)) * kHistPix + (threadIdx.x & 63);
  if (p0 >= img) return;
  const int c0 = blockIdx.y * seg_len, c1 = min(C, c0 + seg_len);
  const float fB = (float)B;
  size_t p[kHistPix];
  float vlo[kHistPix], vsc[kHistPix];
  hist_word P[kHistPix][kHistPlanes];
#pragma unroll
  for (int j = 0; j < kHistPix; ++j) {
    p[j] = p0 + 64 * j < img ? p0 + 64 * j : 0;
    vlo[j] = lo[p[j]];
    vsc[j] = scale[p[j]];
#pragma unroll
    for (int k = 0; k < kHistPlanes; ++k) P[j][k] = 0;
  }
  int c = c0;
  for (; c + 8 <= c1; c += 8) {
    float v[8][kHistPix];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < kHistPix; ++j) v[u][j] = x[(size_t)(c + u) * img + p[j]];
#pragma unroll
    for (int j = 0; j < kHistPix; ++j) {
      hist_word w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = hist_onehot(v[u][j], vlo[j], vsc[j], B, fB);
      hist_add8(P[j], w);
    }
  }
  for (; c < c1; ++c)
#pragma unroll
    for (int j = 0; j < kHistPix; ++j) hist_ripple<0>(P[j], hist_onehot(x[(size_t)c * img + p[j]], vlo[j], vsc[j], B, fB));
#pragma unroll
  for (int j = 0; j < kHistPix; ++j)
    if (p0 + 64 * j < img) hist_flush(P[j], counts, img, p0 + 64 * j);
}

// Chains per segment for a launch of C chains on gx workgroups per segment.  The fewest segments the planes allow, then -- small images only --
// more of them while the launch has fewer than 512 workgroups (two per compute unit) and a segment keeps 128 chains: a flush costs an atomic
// per non-empty row, and at 512 x 512 x 1024 (512 workgroups per segment) one segment takes 0.48 ms where two take 0.60 and four 1.00.
// LMC_HIST_SEG = n (8 .. kHistSeg) fixes the segment length instead: tests reach full-length segments on small images with it, and
// scripts/bench_pixel_hist.py times the choices.
static int hist_segments(int C, int gx) {
  if (const char* e = getenv("LMC_HIST_SEG")) {
    const int n = atoi(e);
    if (n >= 8 && n <= kHistSeg) return (C + n - 1) / n;
  }
  int nseg = (C + kHistSeg - 1) / kHistSeg;
  while ((size_t)gx * nseg < 512 && nseg * 2 <= 65535 && nseg * 256 <= C) nseg *= 2;
  return nseg;
}

// counts[B + 2][H][W] += the histogram of x[C][H][W].  1 <= B <= 62 (the caller checks).  Segments of at most kHistSeg chains go on gridDim.y,
// at most 65535 of them per launch.
hipError_t launch_pixel_hist(const float* x, int64_t C, int H, int W, int B, const float* lo, const float* scale, unsigned long long* counts,
                             hipStream_t st) {
  const size_t img = (size_t)H * W;
  const int gx = (int)((img + 256 * kHistPix - 1) / (256 * kHistPix));
  const int64_t per_launch = (int64_t)8 * 65535;      // every segment length of 8 or more keeps gridDim.y within 65535
  for (int64_t done = 0; done < C; done += per_launch) {
    const int Cl = (int)(C - done < per_launch ? C - done : per_launch);
    const int nseg = hist_segments(Cl, gx);
    const int seg_len = (Cl + nseg - 1) / nseg;
    hipLaunchKernelGGL(pixel_hist_kernel, dim3(gx, nseg), dim3(256), 0, st, x + (size_t)done * img, Cl, img, seg_len, B, lo, scale, counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace lmc
