// The multi-coil SENSE data term: the coil loops around the launchers of lmc_sense_kernel.h (lmc_fft.hip holds those, beside the transforms they share)
// and the host-side bound.  One coil at a time through one spectrum buffer, coils in the order c = 0, 1, ...
#include <cmath>

#include "lmc_launch.h"

namespace lmc {

namespace {

// the planes of the descriptor [1 + 4 n_coils][H][W]
struct SensePlanes {
  const float* d;
  size_t plane;
  int n_coils;
  const float* m() const { return d; }
  const float* s(int c) const { return d + (1 + 2 * (size_t)c) * plane; }
  const float* b(int c) const { return d + (1 + 2 * (size_t)n_coils + 2 * (size_t)c) * plane; }
};

bool sense_ok(const SenseOp& S, int64_t n_img, int H, int W) {
  return S.on && S.desc && S.tw && S.n_coils >= 1 && S.n_coils <= kSenseMaxCoils && n_img >= 1 && fft_shape_ok(H, W);
}

}  // namespace

hipError_t launch_sense_gradient(const SenseOp& S, const float* x, int64_t n_img, int H, int W, hipStream_t st) {
  if (!sense_ok(S, n_img, H, W) || !x || !S.spec || !S.g) return hipErrorInvalidValue;
  const SensePlanes P{S.desc, (size_t)H * W, S.n_coils};
  const int64_t img = (int64_t)H * W;
  for (int c = 0; c < S.n_coils; ++c) {
    hipError_t e = launch_sense_rows_fwd(x, P.s(c), S.spec, img, S.tw, n_img, H, W, st);
    if (e == hipSuccess) e = launch_sense_cols(kSenseGrad, S.spec, img, S.spec, img, P.m(), P.b(c), nullptr, S.tw, n_img, H, W, st);
    if (e == hipSuccess) e = launch_sense_rows_inv(c == 0 ? kSenseStore : kSenseAdd, S.spec, P.s(c), S.g, S.tw, n_img, H, W, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_sense_value(const SenseOp& S, const float* x, int64_t n_img, int H, int W, float sigma_f, double* f_out, hipStream_t st) {
  if (!sense_ok(S, n_img, H, W) || !x || !S.spec || !S.part || !f_out) return hipErrorInvalidValue;
  const SensePlanes P{S.desc, (size_t)H * W, S.n_coils};
  const int64_t img = (int64_t)H * W;
  for (int c = 0; c < S.n_coils; ++c) {
    hipError_t e = launch_sense_rows_fwd(x, P.s(c), S.spec, img, S.tw, n_img, H, W, st);
    if (e == hipSuccess) e = launch_sense_cols(kSenseValue, S.spec, img, S.spec, img, P.m(), P.b(c), S.part, S.tw, n_img, H, W, st);
    if (e == hipSuccess) e = launch_sense_value_finish(S.part, n_img, sense_strips(H, W), 0.5 * (double)sigma_f, f_out, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_sense_apply(const SenseOp& S, const float* in, float* out, int64_t n_img, int H, int W, int adjoint, hipStream_t st) {
  if (!sense_ok(S, n_img, H, W) || !in || !out || (adjoint && !S.spec)) return hipErrorInvalidValue;
  const SensePlanes P{S.desc, (size_t)H * W, S.n_coils};
  const int64_t img = (int64_t)H * W, all = img * S.n_coils;
  for (int c = 0; c < S.n_coils; ++c) {
    hipError_t e;
    if (!adjoint) {      // straight into coil c of every image of the result
      float2* k = reinterpret_cast<float2*>(out) + (size_t)c * img;
      e = launch_sense_rows_fwd(in, P.s(c), k, all, S.tw, n_img, H, W, st);
      if (e == hipSuccess) e = launch_sense_cols(kSenseFwd, k, all, k, all, P.m(), nullptr, nullptr, S.tw, n_img, H, W, st);
    } else {             // the caller's k-space is only read: the column pass writes the spectrum buffer
      const float2* k = reinterpret_cast<const float2*>(in) + (size_t)c * img;
      e = launch_sense_cols(kSenseAdj, k, all, S.spec, img, P.m(), nullptr, nullptr, S.tw, n_img, H, W, st);
      if (e == hipSuccess) e = launch_sense_rows_inv(c == 0 ? kSenseStore : kSenseAdd, S.spec, P.s(c), out, S.tw, n_img, H, W, st);
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

double sense_lipschitz(const float* d, int H, int W, int n_coils) {
  const size_t plane = (size_t)H * W;
  double m2 = 0.0, s2 = 0.0;
  for (size_t p = 0; p < plane; ++p) {
    const double m = d[p];
    m2 = std::fmax(m2, m * m);
    double s = 0.0;
    for (int c = 0; c < n_coils; ++c) {
      const double re = d[(1 + 2 * (size_t)c) * plane + p], im = d[(2 + 2 * (size_t)c) * plane + p];
      s += re * re + im * im;
    }
    s2 = std::fmax(s2, s);
  }
  return m2 * s2;
}

}  // namespace lmc
