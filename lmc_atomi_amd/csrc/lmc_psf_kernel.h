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

#define LMC_PSF_KERNEL_HEAD template <int EPI, bool SEP> __global__ __launch_bounds__(256) void psf_conv_kernel
#include "lmc_psf_conv_body.h"
#undef LMC_PSF_KERNEL_HEAD
// ... and the epilogues of the Huber data term under a name of their own
#define LMC_PSF_KERNEL_HEAD template <int EPI, bool SEP> __global__ __launch_bounds__(256) void psf_hub_kernel
#include "lmc_psf_conv_body.h"
#undef LMC_PSF_KERNEL_HEAD

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
