// The parallel-beam Radon operator: the host side of lmc_radon_kernel.h -- the split of the angles by the axis they walk, the tables, the launchers.
#include <cmath>
#include <cstring>

#include "lmc_radon_kernel.h"

namespace lmc {

namespace {

// the forward kernel walks image rows for this angle (|cos| >= |sin|, compared in float64 as the tables are made)
bool radon_row_kind(float angle) {
  const double th = (double)angle;
  return std::fabs(std::cos(th)) >= std::fabs(std::sin(th));
}

int radon_chunks(const RadonOp& R) {
  return (R.n_row + kRadonAC - 1) / kRadonAC + (R.n_angles - R.n_row + kRadonAC - 1) / kRadonAC;
}

unsigned radon_fwd_blocks(const RadonOp& R) { return (unsigned)(radon_chunks(R) * ((R.n_det + kRadonBins - 1) / kRadonBins)); }

constexpr int64_t kRadonImgChunk = 65535;      // images of one launch: the image index is grid.y

bool radon_ok(const RadonOp& R, int H, int W) {
  return R.on && R.tab_dev && R.n_angles >= 1 && R.n_angles <= kRadonMaxAngles && R.n_det >= 1 && R.n_det <= kRadonMaxDet && H >= 1 && W >= 1 &&
         H <= kRadonMaxSide && W <= kRadonMaxSide;
}

RadonArgs radon_args(const RadonOp& R, int H, int W) {
  RadonArgs A;
  std::memset(&A, 0, sizeof A);
  A.H = H; A.W = W; A.na = R.n_angles; A.nd = R.n_det; A.n_row = R.n_row;
  A.tab = R.tab_dev;
  return A;
}

template <int EPI>
void radon_fwd_one(dim3 grid, const RadonArgs& A, hipStream_t st) {
  hipLaunchKernelGGL((radon_fwd_kernel<EPI>), grid, dim3(kRadonBins), sizeof(float) * (kRadonRed + kRadonLds), st, A);
}

// the forward kernel with epilogue epi on every image, grid.y chunked
hipError_t radon_fwd_all(const RadonOp& R, int epi, RadonArgs A, int64_t n_img, hipStream_t st) {
  const size_t img = (size_t)A.H * A.W, sino = (size_t)A.na * A.nd;
  const unsigned blocks = radon_fwd_blocks(R);
  for (int64_t c0 = 0; c0 < n_img; c0 += kRadonImgChunk) {
    const int64_t nc = n_img - c0 < kRadonImgChunk ? n_img - c0 : kRadonImgChunk;
    RadonArgs B = A;
    B.x = A.x + c0 * img;
    if (A.out) B.out = A.out + c0 * sino;
    if (A.part) B.part = A.part + c0 * blocks;
    const dim3 grid(blocks, (unsigned)nc);
    switch (epi) {
      case kRadonRaw: radon_fwd_one<kRadonRaw>(grid, B, st); break;
      case kRadonRhoL2: radon_fwd_one<kRadonRhoL2>(grid, B, st); break;
      case kRadonRhoPois: radon_fwd_one<kRadonRhoPois>(grid, B, st); break;
      case kRadonRhoWl2: radon_fwd_one<kRadonRhoWl2>(grid, B, st); break;
      case kRadonRhoHub: radon_fwd_one<kRadonRhoHub>(grid, B, st); break;
      case kRadonEnL2: radon_fwd_one<kRadonEnL2>(grid, B, st); break;
      case kRadonEnPois: radon_fwd_one<kRadonEnPois>(grid, B, st); break;
      case kRadonEnWl2: radon_fwd_one<kRadonEnWl2>(grid, B, st); break;
      case kRadonEnHub: radon_fwd_one<kRadonEnHub>(grid, B, st); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

}  // namespace

void radon_prepare(RadonOp& R, const float* angles, int n_angles, int n_det) {
  R.on = 1; R.n_angles = n_angles; R.n_det = n_det;
  std::memcpy(R.angles, angles, sizeof(float) * n_angles);
  int n = 0;
  for (int a = 0; a < n_angles; ++a) if (radon_row_kind(angles[a])) R.order[n++] = a;
  R.n_row = n;
  for (int a = 0; a < n_angles; ++a) if (!radon_row_kind(angles[a])) R.order[n++] = a;
}

size_t radon_table_floats(int n_angles, int H, int W) { return (size_t)n_angles * ((size_t)W + H + 2); }

void radon_tables(const RadonOp& R, int H, int W, float* out) {
#pragma clang fp contract(off)      // products and sums round as written: a checker in float64 reproduces every entry
  const int na = R.n_angles;
  float* ax = out;
  float* by = out + (size_t)na * W;
  float* inv = by + (size_t)na * H;
  const double cx = 0.5 * (W - 1), cy = 0.5 * (H - 1), off = 0.5 * (R.n_det - 1);
  for (int a = 0; a < na; ++a) {
    const double th = (double)R.angles[a], c = std::cos(th), s = std::sin(th);
    for (int j = 0; j < W; ++j) ax[(size_t)a * W + j] = (float)(((double)j - cx) * c);
    for (int i = 0; i < H; ++i) {
      const double ys = ((double)i - cy) * s;
      by[(size_t)a * H + i] = (float)(ys + off);
    }
    inv[a] = (float)(1.0 / (std::fabs(c) >= std::fabs(s) ? c : s));
  }
  std::memcpy(inv + na, R.order, sizeof(int) * na);
}

hipError_t launch_radon_forward(const RadonOp& R, int epi, const float* x, float* out, const float* y, int64_t n_img, int H, int W, hipStream_t st) {
  const bool rho = epi >= kRadonRhoL2 && epi <= kRadonRhoHub;
  if (!radon_ok(R, H, W) || (epi != kRadonRaw && !rho) || !x || !out || n_img < 1 || (rho && !y)) return hipErrorInvalidValue;
  RadonArgs A = radon_args(R, H, W);
  A.x = x; A.out = out; A.y = y;
  return radon_fwd_all(R, epi, A, n_img, st);
}

template <int EPI>
static void radon_adj_one(dim3 grid, const RadonArgs& A, hipStream_t st) {
  hipLaunchKernelGGL((radon_adj_kernel<EPI>), grid, dim3(kRadonTile * kRadonTile), 0, st, A);
}

hipError_t launch_radon_adjoint(const RadonOp& R, int epi, const float* r, float* out, const float* xin, int64_t n_img, int H, int W, float a, float coef,
                                hipStream_t st) {
  if (!radon_ok(R, H, W) || (epi != kRadonRaw && epi != kRadonSub && epi != kRadonOverwrite) || !r || !out || n_img < 1) return hipErrorInvalidValue;
  if (epi == kRadonOverwrite && !xin) return hipErrorInvalidValue;
  RadonArgs A = radon_args(R, H, W);
  A.a = a; A.coef = coef;
  const size_t img = (size_t)H * W, sino = (size_t)R.n_angles * R.n_det;
  const unsigned tiles = (unsigned)(((W + kRadonTile - 1) / kRadonTile) * (size_t)((H + kRadonTile - 1) / kRadonTile));
  for (int64_t c0 = 0; c0 < n_img; c0 += kRadonImgChunk) {
    const int64_t nc = n_img - c0 < kRadonImgChunk ? n_img - c0 : kRadonImgChunk;
    A.x = r + c0 * sino;
    A.out = out + c0 * img;
    A.xin = xin ? xin + c0 * img : nullptr;
    const dim3 grid(tiles, (unsigned)nc);
    switch (epi) {
      case kRadonRaw: radon_adj_one<kRadonRaw>(grid, A, st); break;
      case kRadonSub: radon_adj_one<kRadonSub>(grid, A, st); break;
      default: radon_adj_one<kRadonOverwrite>(grid, A, st); break;
    }
  }
  return hipGetLastError();
}

size_t radon_energy_partials(const RadonOp& R, int64_t n_img) { return (size_t)n_img * radon_fwd_blocks(R); }

hipError_t launch_radon_energy(const RadonOp& R, int term, const float* x, const float* y, int64_t n_img, int H, int W, float sigma_f, double* part,
                               double* f_out, hipStream_t st) {
  if (!radon_ok(R, H, W) || term < 0 || term >= kNumTerms || !x || !y || !part || !f_out || n_img < 1) return hipErrorInvalidValue;
  RadonArgs A = radon_args(R, H, W);
  A.x = x; A.y = y; A.part = part;
  hipError_t e = radon_fwd_all(R, kRadonTermEpi[term].energy, A, n_img, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(radon_energy_finish_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, n_img, (int)radon_fwd_blocks(R),
                     (double)sigma_f, f_out);
  return hipGetLastError();
}

}  // namespace lmc
