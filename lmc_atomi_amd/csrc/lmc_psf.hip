// Large point-spread functions: the host side of lmc_psf_kernel.h -- the separability test, the tap tables of both directions, the launchers.
#include <cmath>
#include <cstring>

#include "lmc_psf_kernel.h"

namespace lmc {

int psf_separable(const float* h, int kh, int kw, float* u, float* v) {
  int pa = 0, pb = 0;
  double best = 0.0;
  for (int a = 0; a < kh; ++a)
    for (int b = 0; b < kw; ++b) {
      const double m = std::fabs((double)h[a * kw + b]);
      if (m > best) { best = m; pa = a; pb = b; }
    }
  if (!(best > 0.0) || !std::isfinite(best)) return 0;       // all zero (or not finite): the general form takes it
  const double piv = (double)h[pa * kw + pb];
  const double tol = std::ldexp(1.0, -22);
  for (int a = 0; a < kh; ++a)
    for (int b = 0; b < kw; ++b) {
      const double hab = (double)h[a * kw + b];
      const double prod = ((double)h[a * kw + pb] / piv) * (double)h[pa * kw + b];
      if (!(std::fabs(prod - hab) <= tol * std::fabs(hab))) return 0;     // (a zero tap: the product must be zero)
    }
  if (u) for (int a = 0; a < kh; ++a) u[a] = (float)((double)h[a * kw + pb] / piv);
  if (v) for (int b = 0; b < kw; ++b) v[b] = h[pa * kw + b];
  return 1;
}

bool psf_prepare(PsfOp& P, const float* h, int kh, int kw, int oy, int ox, int mode) {
  float u[kPsfMax], v[kPsfMax];
  const int sep = mode == 2 ? 0 : psf_separable(h, kh, kw, u, v);
  if (mode == 1 && !sep) return false;
  P.on = 1; P.kh = kh; P.kw = kw; P.oy = oy; P.ox = ox; P.separable = sep;
  std::memset(P.tab, 0, sizeof P.tab);
  float* fwd = P.tab;                             // H: taps flipped, origin mirrored
  float* adj = P.tab + kPsfMax * kPsfKP;          // H^T: taps as given
  if (sep) {
    for (int a = 0; a < kh; ++a) { adj[a] = u[a]; fwd[a] = u[kh - 1 - a]; }
    for (int b = 0; b < kw; ++b) { adj[kPsfKP + b] = v[b]; fwd[kPsfKP + b] = v[kw - 1 - b]; }
  } else {
    for (int a = 0; a < kh; ++a)
      for (int b = 0; b < kw; ++b) {
        adj[b * kPsfKP + a] = h[a * kw + b];
        fwd[b * kPsfKP + a] = h[(kh - 1 - a) * kw + (kw - 1 - b)];
      }
  }
  return true;
}

namespace {

PsfArgs psf_args(const PsfOp& P, int adjoint, int H, int W) {
  PsfArgs A;
  std::memset(&A, 0, sizeof A);
  A.H = H; A.W = W;
  A.tiles_x = (W + kPsfTW - 1) / kPsfTW; A.tiles_y = (H + kPsfTH - 1) / kPsfTH;
  A.kh = P.kh; A.kw = P.kw;
  A.py = adjoint ? P.oy : P.kh - 1 - P.oy;
  A.px = adjoint ? P.ox : P.kw - 1 - P.ox;
  A.g = P.tab_dev + (adjoint ? kPsfMax * kPsfKP : 0);
  return A;
}

// images of one launch: the image index shares grid.x with the tiles
int64_t psf_chunk(const PsfArgs& A) { return 0x7fffffffLL / ((int64_t)A.tiles_x * A.tiles_y); }

template <int EPI>
void psf_launch_one(bool sep, unsigned blocks, const PsfArgs& A, hipStream_t st) {
  if (sep) hipLaunchKernelGGL((psf_conv_kernel<EPI, true>), dim3(blocks), dim3(256), 0, st, A);
  else hipLaunchKernelGGL((psf_conv_kernel<EPI, false>), dim3(blocks), dim3(256), 0, st, A);
}

template <int EPI>      // the Huber epilogues: psf_hub_kernel
void psf_launch_hub(bool sep, unsigned blocks, const PsfArgs& A, hipStream_t st) {
  if (sep) hipLaunchKernelGGL((psf_hub_kernel<EPI, true>), dim3(blocks), dim3(256), 0, st, A);
  else hipLaunchKernelGGL((psf_hub_kernel<EPI, false>), dim3(blocks), dim3(256), 0, st, A);
}

hipError_t psf_launch_all(const PsfOp& P, int epi, PsfArgs A, int64_t n_img, hipStream_t st) {
  if (!P.on || !P.tab_dev || P.kh < 1 || P.kw < 1 || P.kh > kPsfMax || P.kw > kPsfMax) return hipErrorInvalidValue;
  const size_t img = (size_t)A.H * A.W;
  const int64_t tiles = (int64_t)A.tiles_x * A.tiles_y, chunk = psf_chunk(A);
  if (chunk < 1) return hipErrorInvalidValue;
  for (int64_t c0 = 0; c0 < n_img; c0 += chunk) {
    const int64_t nc = n_img - c0 < chunk ? n_img - c0 : chunk;
    PsfArgs B = A;
    B.x = A.x + c0 * img;
    if (A.out) B.out = A.out + c0 * img;
    if (A.xin) B.xin = A.xin + c0 * img;
    if (A.part) B.part = A.part + c0 * tiles;
    const unsigned blocks = (unsigned)(nc * tiles);
    const bool sep = P.separable != 0;
    switch (epi) {
      case kPsfRaw: psf_launch_one<kPsfRaw>(sep, blocks, B, st); break;
      case kPsfRhoL2: psf_launch_one<kPsfRhoL2>(sep, blocks, B, st); break;
      case kPsfRhoWl2: psf_launch_one<kPsfRhoWl2>(sep, blocks, B, st); break;
      case kPsfRhoPois: psf_launch_one<kPsfRhoPois>(sep, blocks, B, st); break;
      case kPsfSub: psf_launch_one<kPsfSub>(sep, blocks, B, st); break;
      case kPsfOverwrite: psf_launch_one<kPsfOverwrite>(sep, blocks, B, st); break;
      case kPsfEnL2: psf_launch_one<kPsfEnL2>(sep, blocks, B, st); break;
      case kPsfEnWl2: psf_launch_one<kPsfEnWl2>(sep, blocks, B, st); break;
      case kPsfEnPois: psf_launch_one<kPsfEnPois>(sep, blocks, B, st); break;
      case kPsfRhoHub: psf_launch_hub<kPsfRhoHub>(sep, blocks, B, st); break;
      case kPsfEnHub: psf_launch_hub<kPsfEnHub>(sep, blocks, B, st); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_psf(const PsfOp& P, int adjoint, int epi, const float* x, float* out, const float* xin, const float* y, int64_t n_img, int H, int W,
                      float a, float coef, hipStream_t st) {
  const bool rho = (epi >= kPsfRhoL2 && epi <= kPsfRhoPois) || epi == kPsfRhoHub;
  if (epi < kPsfRaw || (epi > kPsfOverwrite && !rho) || !x || !out || n_img < 1) return hipErrorInvalidValue;
  if ((epi == kPsfOverwrite && !xin) || (rho && !y)) return hipErrorInvalidValue;
  PsfArgs A = psf_args(P, adjoint, H, W);
  A.x = x; A.out = out; A.xin = xin; A.y = y; A.a = a; A.coef = coef;
  return psf_launch_all(P, epi, A, n_img, st);
}

size_t psf_energy_partials(int64_t n_img, int H, int W) {
  return (size_t)n_img * ((W + kPsfTW - 1) / kPsfTW) * ((H + kPsfTH - 1) / kPsfTH);
}

hipError_t launch_psf_energy(const PsfOp& P, int term, const float* x, const float* y, int64_t n_img, int H, int W, float sigma_f, double* part,
                             double* f_out, hipStream_t st) {
  if (term < 0 || term >= kNumTerms || !x || !y || !part || !f_out || n_img < 1) return hipErrorInvalidValue;
  PsfArgs A = psf_args(P, 0, H, W);
  A.x = x; A.y = y; A.part = part;
  hipError_t e = psf_launch_all(P, kPsfTermEpi[term].energy, A, n_img, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(psf_energy_finish_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, n_img, A.tiles_x * A.tiles_y,
                     (double)sigma_f, f_out);
  return hipGetLastError();
}

}  // namespace lmc
