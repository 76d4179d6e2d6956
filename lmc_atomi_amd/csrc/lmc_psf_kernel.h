// Large point-spread functions (LMC_DATA_PSF, lmc_psf_apply): zero-padded "same" convolution with kernels up to 33 x 33, the operator of lmc_blur.
//
// One workgroup (4 waves) per 32 x 64 output tile and image.  Both directions are ONE correlation form
//     u[i][j] = sum_{a, b} g[a][b] x[i + a - py][j + b - px],       x = 0 outside the image
// with a tap table the host prepares: H^T is g = h, (py, px) = (oy, ox); H is g = h flipped in both directions with the mirrored origin
// (kh - 1 - oy, kw - 1 - ox).  The tile with its halo is staged in LDS with zeros outside the image, so the tap loops carry no bounds tests.  A lane
// owns one column and 8 consecutive rows of the tile: per tap column it slides a 15-row register window down the LDS column, 8 rows of taps at a
// time, so one LDS read feeds 8 FMAs.  The taps come from a device buffer at addresses that do not depend on the lane (scalar loads); the table is
// stored column by column with its rows padded by zeros to a multiple of 8 (kPsfKP floats per column), so that the 8 taps of a block are contiguous.
// Separable kernels (g = gu gv^T): the same sliding window twice.  The column factor first, on every staged column, into a TRANSPOSED second LDS array
// (odd stride: no bank conflicts either way); then the row factor with the lanes remapped to (row, group of 8 columns), so that the window slides along
// the image row; the result returns to the column-per-lane ownership of the epilogue through the (by then free) staging array.
//
// The epilogue is a template parameter: what the three launches of a PSF step and the energies do with u (lmc_psf.hip).
#pragma once
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kPsfTH = 32, kPsfTW = 64;              // output tile
constexpr int kPsfRows = 8;                          // rows per lane = tap rows per block
constexpr int kPsfPH = kPsfTH + kPsfKP - 1;          // staged rows: 71
constexpr int kPsfPW = kPsfTW + kPsfMax - 1;         // staged columns: 96
constexpr int kPsfPW2 = kPsfTW + kPsfKP - 1;         // separable: columns of the intermediate the row window may read (tap columns padded to blocks of 8): 103
constexpr int kPsfST = kPsfTH + 1;                   // separable: stride of the transposed intermediate, [column][row]
constexpr int kPsfSO = kPsfTW + 1;                   // separable: stride of the tile on its way back to the epilogue's ownership
static_assert(kPsfKP % kPsfRows == 0 && kPsfKP >= kPsfMax, "tap rows are padded to whole blocks");
static_assert(kPsfTH == 4 * kPsfRows && kPsfTW == kWave, "4 waves of 64 columns, 8 rows each");
static_assert(kPsfTH == 32 && kPsfTW == 8 * kPsfRows, "separable row pass: 256 lanes = 32 rows x 8 groups of 8 columns");
static_assert(kPsfTH * kPsfSO <= kPsfPH * kPsfPW, "the tile fits the staging array on its way back");

struct PsfArgs {
  const float* x;       // [C][H][W] operand
  float* out;           // [C][H][W]
  const float* xin;     // kPsfOverwrite: [C][H][W]
  const float* y;       // [H][W] or [2][H][W], shared by the images
  const float* g;       // general: g[b * kPsfKP + a]; separable: gu[kPsfKP], then gv[kPsfKP]
  double* part;         // energies: [C][tiles]
  int H, W;
  int tiles_x, tiles_y;
  int kh, kw;
  int py, px;
  float a, coef;
};

// acc[r] += sum_a taps[a] col[(a + r) * stride], a in [0, khp), khp a multiple of 8 (zero taps behind kh); taps at a lane-independent address
__device__ __forceinline__ void psf_column(float (&acc)[kPsfRows], const float* __restrict__ taps, const float* col, int stride, int khp) {
  float w[2 * kPsfRows - 1];
#pragma unroll
  for (int j = 0; j < kPsfRows - 1; ++j) w[j] = col[j * stride];
  for (int a0 = 0; a0 < khp; a0 += kPsfRows) {
#pragma unroll
    for (int j = kPsfRows - 1; j < 2 * kPsfRows - 1; ++j) w[j] = col[(a0 + j) * stride];
#pragma unroll
    for (int j = 0; j < kPsfRows; ++j) {
      const float t = taps[a0 + j];
#pragma unroll
      for (int r = 0; r < kPsfRows; ++r) acc[r] = fmaf(t, w[r + j], acc[r]);
    }
#pragma unroll
    for (int j = 0; j < kPsfRows - 1; ++j) w[j] = w[j + kPsfRows];
  }
}

template <int EPI, bool SEP>
__global__ __launch_bounds__(256) void psf_conv_kernel(PsfArgs P) {
  __shared__ float xs[kPsfPH * kPsfPW];
  __shared__ float hs[SEP ? kPsfPW2 * kPsfST : 1];
  constexpr bool kEnergy = EPI == kPsfEnL2 || EPI == kPsfEnWl2 || EPI == kPsfEnPois;
  __shared__ double red[kEnergy ? 4 : 1];
  const int tid = threadIdx.x, tx = tid & (kWave - 1), wv = tid >> 6;
  const int H = P.H, W = P.W;
  const int tiles = P.tiles_x * P.tiles_y;
  const int im = blockIdx.x / tiles, tile = blockIdx.x - im * tiles;       // the image index shares grid.x with the tiles: any number of images
  const int ty0 = (tile / P.tiles_x) * kPsfTH, tx0 = (tile - (tile / P.tiles_x) * P.tiles_x) * kPsfTW;
  const size_t img = (size_t)H * W;
  const float* __restrict__ xi = P.x + (size_t)im * img;
  const int khp = (P.kh + kPsfRows - 1) / kPsfRows * kPsfRows;
  const int rows = kPsfTH + khp - 1;                 // staged rows the window reads; the rows behind kPsfTH + kh - 1 meet zero taps only
  for (int e = tid; e < rows * kPsfPW; e += 256) {
    const int r = e / kPsfPW, c = e - r * kPsfPW;
    const int gr = ty0 + r - P.py, gc = tx0 + c - P.px;
    const bool in = r < kPsfTH + P.kh - 1 && c < kPsfTW + P.kw - 1 && gr >= 0 && gr < H && gc >= 0 && gc < W;
    xs[e] = in ? xi[(size_t)gr * W + gc] : 0.f;
  }
  __syncthreads();
  float acc[kPsfRows];
#pragma unroll
  for (int r = 0; r < kPsfRows; ++r) acc[r] = 0.f;
  const float* __restrict__ g = P.g;
  if constexpr (SEP) {
    const int kwp = (P.kw + kPsfRows - 1) / kPsfRows * kPsfRows;
    const int ncols = kPsfTW + P.kw - 1;             // staged columns that carry data; the row window reads up to kPsfTW + kwp - 1: zeros behind ncols
    for (int e = tid; e < (kPsfTW + kwp - 1 - ncols) * kPsfTH; e += 256) hs[(ncols + e / kPsfTH) * kPsfST + (e & (kPsfTH - 1))] = 0.f;
    for (int c = tx; c < ncols; c += kPsfTW) {       // column factor: hs[c][i] = sum_a gu[a] xs[i + a][c], the lane's 8 rows of column c
      float v[kPsfRows];
#pragma unroll
      for (int r = 0; r < kPsfRows; ++r) v[r] = 0.f;
      psf_column(v, g, xs + wv * kPsfRows * kPsfPW + c, kPsfPW, khp);
#pragma unroll
      for (int r = 0; r < kPsfRows; ++r) hs[c * kPsfST + wv * kPsfRows + r] = v[r];
    }
    __syncthreads();
    const int hr = tid & (kPsfTH - 1), cg = tid >> 5;     // row factor: the lane's row and its 8 columns cg * 8 .. + 7
    float o[kPsfRows];
#pragma unroll
    for (int j = 0; j < kPsfRows; ++j) o[j] = 0.f;
    psf_column(o, g + kPsfKP, hs + cg * kPsfRows * kPsfST + hr, kPsfST, kwp);
#pragma unroll
    for (int j = 0; j < kPsfRows; ++j) xs[hr * kPsfSO + cg * kPsfRows + j] = o[j];      // (every read of the staged tile lies before the barrier above)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPsfRows; ++r) acc[r] = xs[(wv * kPsfRows + r) * kPsfSO + tx];
  } else {
    for (int b = 0; b < P.kw; ++b) psf_column(acc, g + b * kPsfKP, xs + wv * kPsfRows * kPsfPW + tx + b, kPsfPW, khp);
  }
  const int gc = tx0 + tx;
  double fa = 0.0;
#pragma unroll
  for (int r = 0; r < kPsfRows; ++r) {
    const int gr = ty0 + wv * kPsfRows + r;
    if (gr < H && gc < W) {
      const size_t p = (size_t)gr * W + gc, o = (size_t)im * img + p;
      const float u = acc[r];
      if constexpr (EPI == kPsfRaw) P.out[o] = u;
      if constexpr (EPI == kPsfRhoL2) P.out[o] = u - P.y[p];
      if constexpr (EPI == kPsfRhoWl2) P.out[o] = P.y[img + p] * (u - P.y[p]);
      if constexpr (EPI == kPsfRhoPois) P.out[o] = pois_rho(u, P.y[p], P.y[img + p]);
      if constexpr (EPI == kPsfSub) P.out[o] = fmaf(-P.coef, u, P.out[o]);
      if constexpr (EPI == kPsfOverwrite) P.out[o] = fmaf(-P.coef, u, P.a * P.xin[o]);
      if constexpr (EPI == kPsfEnL2) { const double d = (double)u - (double)P.y[p]; fa += 0.5 * d * d; }
      if constexpr (EPI == kPsfEnWl2) { const double d = (double)u - (double)P.y[p]; fa += 0.5 * (double)P.y[img + p] * d * d; }
      if constexpr (EPI == kPsfEnPois) fa += pois_phi(u, P.y[p], P.y[img + p]);
    }
  }
  if constexpr (kEnergy) {      // a fixed order: lanes by shuffles, then the four waves by thread 0 -- no atomics, equal from run to run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) fa += __shfl_down(fa, off, kWave);
    if (tx == 0) red[wv] = fa;
    __syncthreads();
    if (tid == 0) P.part[(size_t)im * tiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// f_out[c] += scale * sum_t part[c][t], t in order: one lane per image
__global__ __launch_bounds__(256) void psf_energy_finish_kernel(const double* __restrict__ part, int64_t n_img, int tiles, double scale,
                                                                double* __restrict__ f_out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_img) return;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += part[(size_t)c * tiles + t];
  f_out[c] += scale * s;
}

}  // namespace lmc
