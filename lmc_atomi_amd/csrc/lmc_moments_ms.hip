// Multi-scale posterior moments: one pass over a kept iterate that updates the pixel accumulators s1, s2 (as moments4_kernel does) and, for
// every enabled scale s in {2, 4, 8, 16}, S2_s[block] += (sum of the block's pixels of ONE chain)^2 -- the second moment of the block sums,
// which no pixel-wise accumulator can give.  (S1_s is the block sum of the pixel s1: block_sums_kernel forms it when it is asked for.)
// Every block sum is formed in float64 from the fp32 pixels: the images have a mean 100x their spread, where an fp32 block sum would cost
// 1 % of the variance.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

// A wave owns a tile of 16 rows x 32 columns; lane = 8 * rr + pc holds the 2 x 4 pixels at rows 2 rr, 2 rr + 1, columns 4 pc .. 4 pc + 3
// (two 16-byte loads per chain: eight lanes read 128 contiguous bytes of a row).  The 2 x 2 blocks and the 4-wide half of a 4 x 4 block are
// sums inside the lane; 4 x 4 needs lane ^ 8, 8 x 8 lanes ^ 1 and ^ 16, 16 x 16 lanes ^ 2 and ^ 32 -- ds_bpermute shuffles, no LDS
// allocation (the reason is written above moments4_kernel).  Every lane of a block ends up with the block's sum and squares it into its own
// accumulator; the lane at the block's origin issues the one atomic per block and chain segment.
// Lanes outside the image (partial tiles) read pixel 0 of the chain and keep zeros: the shuffles need every lane in the loop.
template <int U>
__device__ __forceinline__ void ms_reduce_tile(const float* __restrict__ x, int cs, int ce, size_t img, int H, int W, int ty, int tx,
                                               double* __restrict__ s1, double* __restrict__ s2, const BlockScales& B) {
  const int lane = threadIdx.x & 63;
  const int rr = lane >> 3, pc = lane & 7;
  const int y = ty * 16 + 2 * rr, xc = tx * 32 + 4 * pc;
  const bool in0 = xc < W && y < H, in1 = xc < W && y + 1 < H;
  const float* __restrict__ p0 = x + (in0 ? (size_t)y * W + xc : 0);
  const float* __restrict__ p1 = x + (in1 ? (size_t)(y + 1) * W + xc : 0);
  double a[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, b[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  double q2[2] = {0.0, 0.0}, q4 = 0.0, q8 = 0.0, q16 = 0.0;
  auto add_chain = [&](float4 v0, float4 v1) {
    const double d0[4] = {in0 ? (double)v0.x : 0.0, in0 ? (double)v0.y : 0.0, in0 ? (double)v0.z : 0.0, in0 ? (double)v0.w : 0.0};
    const double d1[4] = {in1 ? (double)v1.x : 0.0, in1 ? (double)v1.y : 0.0, in1 ? (double)v1.z : 0.0, in1 ? (double)v1.w : 0.0};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      a[0][m] += d0[m]; a[1][m] += d1[m];
      b[0][m] = fma(d0[m], d0[m], b[0][m]); b[1][m] = fma(d1[m], d1[m], b[1][m]);
    }
    const double h0 = (d0[0] + d0[1]) + (d1[0] + d1[1]), h1 = (d0[2] + d0[3]) + (d1[2] + d1[3]);   // the lane's two 2 x 2 blocks
    q2[0] = fma(h0, h0, q2[0]); q2[1] = fma(h1, h1, q2[1]);
    double t = h0 + h1;                                   // 4 wide, 2 tall
    t += __shfl_xor(t, 8, 64);                            // 4 x 4
    q4 = fma(t, t, q4);
    t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 16, 64);   // 8 x 8
    q8 = fma(t, t, q8);
    t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 32, 64);   // 16 x 16
    q16 = fma(t, t, q16);
  };
  int c = cs;
  for (; c + U <= ce; c += U) {
    float4 v0[U], v1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v0[u] = *reinterpret_cast<const float4*>(p0 + (size_t)(c + u) * img);
      v1[u] = *reinterpret_cast<const float4*>(p1 + (size_t)(c + u) * img);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) add_chain(v0[u], v1[u]);
  }
  for (; c < ce; ++c)
    add_chain(*reinterpret_cast<const float4*>(p0 + (size_t)c * img), *reinterpret_cast<const float4*>(p1 + (size_t)c * img));

  // pixel accumulators, lane-contiguous as in moments4_kernel: atomic (k, i) of lane l covers pixel l & 31 of the tile's row 2 (2 i + l / 32) + k
  // -- two runs of 256 contiguous bytes per wave instruction -- which is component l & 3 of lane 8 (2 i + l / 32) + (l & 31) / 4.
  const int sel = lane & 3;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int srr = 2 * i + (lane >> 5);
      const int srcl = 8 * srr + ((lane & 31) >> 2);
      double va = 0.0, vb = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const double ta = __shfl(a[k][m], srcl, 64), tb = __shfl(b[k][m], srcl, 64);
        if (sel == m) { va = ta; vb = tb; }
      }
      const int row = ty * 16 + 2 * srr + k, col = tx * 32 + (lane & 31);
      if (row < H && col < W) {
        const size_t q = (size_t)row * W + col;
        unsafeAtomicAdd(&s1[q], va);
        unsafeAtomicAdd(&s2[q], vb);
      }
    }
  // block accumulators [ceil(H / s)][ceil(W / s)]: a block whose origin is inside the image is inside the array
  if (B.s2[0]) {   // 2 x 2: atomic j of lane pc covers block 8 j + pc of the lane group's 16: component pc & 1 of the group's lane 4 j + pc / 2
    const int bw = (W + 1) >> 1, bh = (H + 1) >> 1, br = ty * 8 + rr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int srcl = (lane & ~7) + 4 * j + (pc >> 1);
      const double t0 = __shfl(q2[0], srcl, 64), t1 = __shfl(q2[1], srcl, 64);
      const int bc = tx * 16 + 8 * j + pc;
      if (br < bh && bc < bw) unsafeAtomicAdd(&B.s2[0][(size_t)br * bw + bc], (pc & 1) ? t1 : t0);
    }
  }
  if (B.s2[1] && !(rr & 1)) {
    const int bw = (W + 3) >> 2, bh = (H + 3) >> 2, br = ty * 4 + (rr >> 1), bc = tx * 8 + pc;
    if (br < bh && bc < bw) unsafeAtomicAdd(&B.s2[1][(size_t)br * bw + bc], q4);
  }
  if (B.s2[2] && !(rr & 3) && !(pc & 1)) {
    const int bw = (W + 7) >> 3, bh = (H + 7) >> 3, br = ty * 2 + (rr >> 2), bc = tx * 4 + (pc >> 1);
    if (br < bh && bc < bw) unsafeAtomicAdd(&B.s2[2][(size_t)br * bw + bc], q8);
  }
  if (B.s2[3] && !rr && !(pc & 3)) {
    const int bw = (W + 15) >> 4, bh = (H + 15) >> 4, br = ty, bc = tx * 2 + (pc >> 2);
    if (br < bh && bc < bw) unsafeAtomicAdd(&B.s2[3][(size_t)br * bw + bc], q16);
  }
}

// In line: one tile per wave, grid.y = chain segments (the twin of moments4_kernel).  W % 4 == 0.
__global__ __launch_bounds__(256) void moments_ms_kernel(const float* __restrict__ x, int C, int H, int W, int seg_len, int tiles_x, int n_tiles,
                                                         double* __restrict__ s1, double* __restrict__ s2, BlockScales B) {
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;                 // the whole wave leaves
  const int cs = blockIdx.y * seg_len;
  ms_reduce_tile<4>(x, cs, min(C, cs + seg_len), (size_t)H * W, H, W, tile / tiles_x, tile % tiles_x, s1, s2, B);
}

// Paced, for the side stream: gridDim.x workgroups walking the groups of four tiles (the twin of moments4_bg_kernel).  Two chains in flight
// instead of four keeps the wave inside what the one-team pipe kernel leaves of a SIMD's registers.
__global__ __launch_bounds__(256) void moments_ms_bg_kernel(const float* __restrict__ x, int C, int H, int W, int tiles_x, int n_tiles,
                                                            double* __restrict__ s1, double* __restrict__ s2, BlockScales B) {
  const int seg_len = (C + (int)gridDim.y - 1) / (int)gridDim.y;
  const int cs = (int)blockIdx.y * seg_len, ce = min(C, cs + seg_len);
  for (int g = blockIdx.x; g * 4 < n_tiles; g += gridDim.x) {
    const int tile = g * 4 + (threadIdx.x >> 6);
    if (tile < n_tiles) ms_reduce_tile<2>(x, cs, ce, (size_t)H * W, H, W, tile / tiles_x, tile % tiles_x, s1, s2, B);
  }
}

// Any width: one thread per 16 x 16 block walks its pixels, then its blocks of every enabled scale, chain by chain; one atomic per pixel or
// block and chain segment.  Plain on purpose: the re-reads come from cache, and widths that are no multiple of 4 are not what the samplers are sized for.
__global__ __launch_bounds__(256) void moments_ms_generic_kernel(const float* __restrict__ x, int C, int H, int W, int seg_len,
                                                                 double* __restrict__ s1, double* __restrict__ s2, BlockScales B) {
  const int bw16 = (W + 15) >> 4, bh16 = (H + 15) >> 4;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= bw16 * bh16) return;
  const int y0 = (t / bw16) * 16, x0 = (t % bw16) * 16, y1 = min(H, y0 + 16), x1 = min(W, x0 + 16);
  const size_t img = (size_t)H * W;
  const int cs = blockIdx.y * seg_len, ce = min(C, cs + seg_len);
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) {
      const size_t p = (size_t)yy * W + xx;
      double a = 0.0, b = 0.0;
      for (int c = cs; c < ce; ++c) {
        const double v = (double)x[(size_t)c * img + p];
        a += v;
        b = fma(v, v, b);
      }
      unsafeAtomicAdd(&s1[p], a);
      unsafeAtomicAdd(&s2[p], b);
    }
  for (int si = 0; si < 4; ++si) {
    if (!B.s2[si]) continue;
    const int s = 2 << si, bw = (W + s - 1) / s;
    for (int by = y0; by < y1; by += s)
      for (int bx = x0; bx < x1; bx += s) {
        const int ey = min(by + s, y1), ex = min(bx + s, x1);
        double q = 0.0;
        for (int c = cs; c < ce; ++c) {
          const float* __restrict__ xc = x + (size_t)c * img;
          double v = 0.0;
          for (int yy = by; yy < ey; ++yy)
            for (int xx = bx; xx < ex; ++xx) v += (double)xc[(size_t)yy * W + xx];
          q = fma(v, v, q);
        }
        unsafeAtomicAdd(&B.s2[si][(size_t)(by / s) * bw + bx / s], q);
      }
  }
}

// out[i][j] = sum of the block (i, j) of scale s of `src` ([H][W] doubles): S1_s from the pixel s1
__global__ __launch_bounds__(256) void block_sums_kernel(const double* __restrict__ src, int H, int W, int s, double* __restrict__ out) {
  const int bw = (W + s - 1) / s, bh = (H + s - 1) / s;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= bw * bh) return;
  const int y0 = (t / bw) * s, x0 = (t % bw) * s, y1 = min(H, y0 + s), x1 = min(W, x0 + s);
  double v = 0.0;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) v += src[(size_t)yy * W + xx];
  out[t] = v;
}

static hipError_t launch_ms_generic(const float* x, int C, int H, int W, double* s1, double* s2, const BlockScales& B, hipStream_t st) {
  const int gx = (((W + 15) >> 4) * ((H + 15) >> 4) + 255) / 256;
  int nseg = 1;
  while ((size_t)gx * nseg < 2048 && nseg * 2 <= C) nseg *= 2;     // few threads, each with a whole 16 x 16 block: split the chains finely
  const int seg_len = (C + nseg - 1) / nseg;
  hipLaunchKernelGGL(moments_ms_generic_kernel, dim3(gx, nseg), dim3(256), 0, st, x, C, H, W, seg_len, s1, s2, B);
  return hipGetLastError();
}

hipError_t launch_moments_ms(const float* x, int C, int H, int W, double* s1, double* s2, const BlockScales& B, hipStream_t st) {
  if (W & 3) return launch_ms_generic(x, C, H, W, s1, s2, B, st);
  const int tiles_x = (W + 31) >> 5, n_tiles = tiles_x * ((H + 15) >> 4);
  const int gx = (n_tiles + 3) / 4;
  int nseg = 1;
  while ((size_t)gx * nseg < 2048 && nseg * 16 <= C) nseg *= 2;
  const int seg_len = (C + nseg - 1) / nseg;
  hipLaunchKernelGGL(moments_ms_kernel, dim3(gx, nseg), dim3(256), 0, st, x, C, H, W, seg_len, tiles_x, n_tiles, s1, s2, B);
  return hipGetLastError();
}

// same result as launch_moments_ms, paced: `n_wg` workgroups in total (W % 4 == 0 required, else falls back to launch_moments_ms)
hipError_t launch_moments_ms_bg(const float* x, int C, int H, int W, double* s1, double* s2, const BlockScales& B, int n_wg, hipStream_t st) {
  if ((W & 3) || n_wg < 1) return launch_moments_ms(x, C, H, W, s1, s2, B, st);
  const int tiles_x = (W + 31) >> 5, n_tiles = tiles_x * ((H + 15) >> 4);
  const int n_groups = (n_tiles + 3) / 4;
  int nseg = 1;
  if (n_wg > n_groups) {        // fewer tile groups than workgroups asked for: split the chains as well (>= 16 chains per segment)
    while (n_groups * nseg * 2 <= n_wg && nseg * 32 <= C) nseg *= 2;
    n_wg = n_groups;
  }
  hipLaunchKernelGGL(moments_ms_bg_kernel, dim3(n_wg, nseg), dim3(256), 0, st, x, C, H, W, tiles_x, n_tiles, s1, s2, B);
  return hipGetLastError();
}

hipError_t launch_block_sums(const double* src, int H, int W, int scale, double* out, hipStream_t st) {
  const int n = ((W + scale - 1) / scale) * ((H + scale - 1) / scale);
  hipLaunchKernelGGL(block_sums_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, H, W, scale, out);
  return hipGetLastError();
}

}  // namespace lmc
