// The spectral data term: the host side of lmc_fft_kernel.h -- the twiddle table, the folded descriptor planes, the launchers.
#include <cmath>
#include <cstring>

#include "lmc_fft_kernel.h"
#include "lmc_sense_kernel.h"
#include "lmc_sgs_kernel.h"

namespace lmc {

namespace {

int fft_log2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

size_t fft_lds_bytes(int N) { return 2 * (size_t)(kFftElems / N) * fft_line_stride(N) * sizeof(float2); }

// more than 64 KiB of LDS for the short lines (many lines, one pad slot each): raised once per kernel and device
template <auto kern, class Args>
hipError_t fft_launch(unsigned blocks, size_t lds, const Args& A, hipStream_t st) {
  static bool attr_set[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds_bytes(kFftMin));
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kFftThreads), lds, st, A);
  return hipGetLastError();
}

FftArgs fft_args(const float2* tw, int64_t n_img, int H, int W) {
  FftArgs A;
  std::memset(&A, 0, sizeof A);
  A.tw = tw;
  A.rows = n_img * H;
  A.H = H; A.W = W; A.Wh = W / 2 + 1;
  A.logH = fft_log2(H); A.logW = fft_log2(W);
  return A;
}

// strips of one image and the images of one launch (the image index shares grid.x with the strips)
int fft_strips(int H, int W) { const int cw = kFftElems / H; return (W / 2 + 1 + cw - 1) / cw; }
int64_t fft_chunk(int strips) { return 0x7fffffffLL / strips; }

template <int MODE>
hipError_t fft_cols_one(unsigned blocks, size_t lds, const FftArgs& A, hipStream_t st) {
  return fft_launch<fft_cols_spectral_kernel<MODE>>(blocks, lds, A, st);
}

hipError_t fft_cols_all(int mode, FftArgs A, int64_t n_img, hipStream_t st) {
  A.lines = kFftElems / A.H;
  A.strips = fft_strips(A.H, A.W);
  const size_t lds = fft_lds_bytes(A.H), img = (size_t)A.H * A.Wh;
  const int64_t chunk = fft_chunk(A.strips);
  for (int64_t c0 = 0; c0 < n_img; c0 += chunk) {
    const int64_t nc = n_img - c0 < chunk ? n_img - c0 : chunk;
    FftArgs B = A;
    B.spec = A.spec + c0 * img;
    if (A.part) B.part = A.part + c0 * A.strips;
    const unsigned blocks = (unsigned)(nc * A.strips);
    hipError_t e;
    switch (mode) {
      case kFftColFwd: e = fft_cols_one<kFftColFwd>(blocks, lds, B, st); break;
      case kFftColInv: e = fft_cols_one<kFftColInv>(blocks, lds, B, st); break;
      case kFftGrad: e = fft_cols_one<kFftGrad>(blocks, lds, B, st); break;
      case kFftProx: e = fft_cols_one<kFftProx>(blocks, lds, B, st); break;
      case kFftMul: e = fft_cols_one<kFftMul>(blocks, lds, B, st); break;
      case kFftValue: e = fft_cols_one<kFftValue>(blocks, lds, B, st); break;
      default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

bool fft_shape_ok(int H, int W) {
  return H >= kFftMin && H <= kFftMax && W >= kFftMin && W <= kFftMax && !(H & (H - 1)) && !(W & (W - 1));
}

void fft_twiddles(float* tw) {
  const double pi = 3.14159265358979323846;
  for (int m = 0; m < kFftTw; ++m) {
    const double ang = -2.0 * pi * (double)m / (double)kFftTw;
    tw[2 * m] = (float)std::cos(ang);
    tw[2 * m + 1] = (float)std::sin(ang);
  }
  // the four axis points exactly
  tw[0] = 1.f; tw[1] = 0.f;
  tw[2 * (kFftTw / 4)] = 0.f; tw[2 * (kFftTw / 4) + 1] = -1.f;
  tw[2 * (kFftTw / 2)] = -1.f; tw[2 * (kFftTw / 2) + 1] = 0.f;
  tw[2 * (3 * kFftTw / 4)] = 0.f; tw[2 * (3 * kFftTw / 4) + 1] = 1.f;
}

size_t fft_spec_floats(int64_t n_img, int H, int W) { return 2 * (size_t)n_img * H * (W / 2 + 1); }
size_t fft_value_partials(int64_t n_img, int H, int W) { return (size_t)n_img * fft_strips(H, W); }

void fft_tables(const double* G, const double* b, int H, int W, float* out) {
  const int Wh = W / 2 + 1;
  const size_t plane = (size_t)H * Wh;
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < Wh; ++j) {
      const size_t k = (size_t)i * W + j, m = (size_t)((H - i) % H) * W + (size_t)((W - j) % W);
      const double gr = G[2 * k], gi = G[2 * k + 1], br = b[2 * k], bi = b[2 * k + 1];
      const double hr = G[2 * m], hi = G[2 * m + 1], dr = b[2 * m], di = b[2 * m + 1];     // at -k
      float* o = out + (size_t)i * Wh + j;
      o[0] = (float)(0.5 * (gr * gr + gi * gi + hr * hr + hi * hi));
      // conj(G_k) b_k + G_-k conj(b_-k)
      o[plane] = (float)(0.5 * ((gr * br + gi * bi) + (hr * dr + hi * di)));
      o[2 * plane] = (float)(0.5 * ((gr * bi - gi * br) + (hi * dr - hr * di)));
      o[3 * plane] = (float)gr; o[4 * plane] = (float)gi;
      o[5 * plane] = (float)br; o[6 * plane] = (float)bi;
      const bool self = j == 0 || 2 * j == W;      // -k is visited by the half plane itself
      o[7 * plane] = self ? 0.f : (float)hr; o[8 * plane] = self ? 0.f : (float)-hi;
      o[9 * plane] = self ? 0.f : (float)dr; o[10 * plane] = self ? 0.f : (float)-di;
    }
}

hipError_t launch_fft_rows_fwd(const float* x, float2* spec, const float2* tw, int64_t n_img, int H, int W, hipStream_t st) {
  if (!x || !spec || !tw || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  FftArgs A = fft_args(tw, n_img, H, W);
  A.x = x; A.spec = spec;
  A.lines = kFftElems / W;
  const int64_t blocks = (A.rows + A.lines - 1) / A.lines;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  return fft_launch<fft_rows_fwd_kernel>((unsigned)blocks, fft_lds_bytes(W), A, st);
}

hipError_t launch_fft_cols(int mode, float2* spec, const float* tab, const float2* tw, int64_t n_img, int H, int W, float ts, hipStream_t st) {
  if (mode < kFftColFwd || mode > kFftMul || !spec || !tw || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  if (mode >= kFftGrad && !tab) return hipErrorInvalidValue;
  FftArgs A = fft_args(tw, n_img, H, W);
  A.spec = spec; A.tab = tab; A.ts = ts;
  return fft_cols_all(mode, A, n_img, st);
}

hipError_t launch_fft_gibbs(float2* zspec, const float2* nspec, const float* tab, const float2* tw, int64_t n_img, int H, int W, float rinv, float sf,
                            hipStream_t st) {
  if (!zspec || !tab || !tw || zspec == nspec || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  SgsColsArgs A;
  std::memset(&A, 0, sizeof A);
  A.tw = tw; A.tab = tab; A.rinv = rinv; A.sf = sf;
  A.H = H; A.Wh = W / 2 + 1; A.logH = fft_log2(H);
  A.lines = kFftElems / H;
  A.strips = fft_strips(H, W);
  const size_t img = (size_t)H * A.Wh;
  const int64_t chunk = fft_chunk(A.strips);
  for (int64_t c0 = 0; c0 < n_img; c0 += chunk) {
    const int64_t nc = n_img - c0 < chunk ? n_img - c0 : chunk;
    A.zspec = zspec + c0 * img;
    A.nspec = nspec ? nspec + c0 * img : nullptr;
    const hipError_t e = fft_launch<sgs_cols_gibbs_kernel>((unsigned)(nc * A.strips), fft_lds_bytes(H), A, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_fft_rows_inv(int epi, const float2* spec, float* out, const float* xin, const float2* tw, int64_t n_img, int H, int W, float a, float coef,
                               hipStream_t st) {
  if (epi < kFftStore || epi > kFftOverwrite || !spec || !out || !tw || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  if (epi == kFftOverwrite && !xin) return hipErrorInvalidValue;
  FftArgs A = fft_args(tw, n_img, H, W);
  A.spec = const_cast<float2*>(spec); A.out = out; A.x = xin; A.a = a; A.coef = coef;
  A.lines = kFftElems / W;
  const int64_t blocks = (A.rows + A.lines - 1) / A.lines;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = fft_lds_bytes(W);
  switch (epi) {
    case kFftStore: return fft_launch<fft_rows_inv_kernel<kFftStore>>((unsigned)blocks, lds, A, st);
    case kFftSub: return fft_launch<fft_rows_inv_kernel<kFftSub>>((unsigned)blocks, lds, A, st);
    default: return fft_launch<fft_rows_inv_kernel<kFftOverwrite>>((unsigned)blocks, lds, A, st);
  }
}

hipError_t launch_fft_value(const FftOp& F, const float* x, int64_t n_img, int H, int W, float sigma_f, double* f_out, hipStream_t st) {
  if (!F.on || !F.tab || !F.tw || !F.spec || !F.part || !x || !f_out || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  hipError_t e = launch_fft_rows_fwd(x, F.spec, F.tw, n_img, H, W, st);
  if (e != hipSuccess) return e;
  FftArgs A = fft_args(F.tw, n_img, H, W);
  A.spec = F.spec; A.part = F.part;
  A.tab = F.tab + 3 * (size_t)H * A.Wh;
  e = fft_cols_all(kFftValue, A, n_img, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fft_value_finish_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, F.part, n_img, fft_strips(H, W),
                     0.5 * (double)sigma_f, f_out);
  return hipGetLastError();
}

// ---- the launchers of lmc_sense_kernel.h (the coil loops around them: lmc_sense.hip) ----

namespace {

SenseArgs sense_args(const float2* tw, int64_t n_img, int H, int W) {
  SenseArgs A;
  std::memset(&A, 0, sizeof A);
  A.tw = tw;
  A.rows = n_img * H;
  A.H = H; A.W = W;
  A.logH = fft_log2(H); A.logW = fft_log2(W);
  return A;
}

template <int MODE>
hipError_t sense_cols_one(unsigned blocks, size_t lds, const SenseArgs& A, hipStream_t st) {
  return fft_launch<sense_cols_kernel<MODE>>(blocks, lds, A, st);
}

}  // namespace

int sense_strips(int H, int W) { const int cw = kFftElems / H; return (W + cw - 1) / cw; }
size_t sense_spec_floats(int64_t n_img, int H, int W) { return 2 * (size_t)n_img * H * W; }
size_t sense_value_partials(int64_t n_img, int H, int W) { return (size_t)n_img * sense_strips(H, W); }

hipError_t launch_sense_rows_fwd(const float* x, const float* s, float2* spec, int64_t spec_stride, const float2* tw, int64_t n_img, int H, int W, hipStream_t st) {
  if (!x || !s || !spec || !tw || n_img < 1 || !fft_shape_ok(H, W) || spec_stride < (int64_t)H * W) return hipErrorInvalidValue;
  SenseArgs A = sense_args(tw, n_img, H, W);
  A.x = x; A.s = s; A.spec = spec; A.spec_stride = spec_stride;
  A.lines = kFftElems / W;
  const int64_t blocks = (A.rows + A.lines - 1) / A.lines;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  return fft_launch<sense_rows_fwd_kernel>((unsigned)blocks, fft_lds_bytes(W), A, st);
}

hipError_t launch_sense_cols(int mode, const float2* src, int64_t src_stride, float2* spec, int64_t spec_stride, const float* m, const float* b, double* part,
                             const float2* tw, int64_t n_img, int H, int W, hipStream_t st) {
  if (mode < kSenseGrad || mode > kSenseAdj || !src || !spec || !m || !tw || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  if (src_stride < (int64_t)H * W || spec_stride < (int64_t)H * W) return hipErrorInvalidValue;
  if ((mode == kSenseGrad || mode == kSenseValue) && !b) return hipErrorInvalidValue;
  if (mode == kSenseValue && !part) return hipErrorInvalidValue;
  SenseArgs A = sense_args(tw, n_img, H, W);
  A.m = m; A.b = b;
  A.src_stride = src_stride; A.spec_stride = spec_stride;
  A.lines = kFftElems / H;
  A.strips = sense_strips(H, W);
  const size_t lds = fft_lds_bytes(H);
  const int64_t chunk = fft_chunk(A.strips);
  for (int64_t c0 = 0; c0 < n_img; c0 += chunk) {      // the image index shares grid.x with the strips
    const int64_t nc = n_img - c0 < chunk ? n_img - c0 : chunk;
    A.src = src + c0 * src_stride;
    A.spec = spec + c0 * spec_stride;
    A.part = part ? part + c0 * A.strips : nullptr;
    const unsigned blocks = (unsigned)(nc * A.strips);
    hipError_t e;
    switch (mode) {
      case kSenseGrad: e = sense_cols_one<kSenseGrad>(blocks, lds, A, st); break;
      case kSenseValue: e = sense_cols_one<kSenseValue>(blocks, lds, A, st); break;
      case kSenseFwd: e = sense_cols_one<kSenseFwd>(blocks, lds, A, st); break;
      default: e = sense_cols_one<kSenseAdj>(blocks, lds, A, st); break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_sense_rows_inv(int epi, const float2* spec, const float* s, float* out, const float2* tw, int64_t n_img, int H, int W, hipStream_t st) {
  if (epi < kSenseStore || epi > kSenseAdd || !spec || !s || !out || !tw || n_img < 1 || !fft_shape_ok(H, W)) return hipErrorInvalidValue;
  SenseArgs A = sense_args(tw, n_img, H, W);
  A.spec = const_cast<float2*>(spec); A.s = s; A.out = out;
  A.lines = kFftElems / W;
  const int64_t blocks = (A.rows + A.lines - 1) / A.lines;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = fft_lds_bytes(W);
  if (epi == kSenseStore) return fft_launch<sense_rows_inv_kernel<kSenseStore>>((unsigned)blocks, lds, A, st);
  return fft_launch<sense_rows_inv_kernel<kSenseAdd>>((unsigned)blocks, lds, A, st);
}

hipError_t launch_sense_value_finish(const double* part, int64_t n_img, int strips, double scale, double* f_out, hipStream_t st) {
  if (!part || !f_out || n_img < 1 || strips < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fft_value_finish_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, n_img, strips, scale, f_out);
  return hipGetLastError();
}

hipError_t launch_sense_axpy(bool alone, const float* g, const float* x, float* out, size_t n, float a, float coef, hipStream_t st) {
  if (!g || !out || (alone && !x) || n < 1) return hipErrorInvalidValue;
  const size_t want = (n + 255) / 256;
  const unsigned blocks = (unsigned)(want < ((size_t)1 << 20) ? want : ((size_t)1 << 20));
  if (alone) hipLaunchKernelGGL(sense_axpy_kernel<true>, dim3(blocks), dim3(256), 0, st, g, x, out, n, a, coef);
  else hipLaunchKernelGGL(sense_axpy_kernel<false>, dim3(blocks), dim3(256), 0, st, g, x, out, n, a, coef);
  return hipGetLastError();
}

}  // namespace lmc
