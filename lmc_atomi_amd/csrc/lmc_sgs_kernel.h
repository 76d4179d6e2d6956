// The column pass of the split Gibbs sampler's spectral x-draw (include/lmc_atomi.h, lmc_sgs_*): a kernel of its own beside fft_cols_spectral_kernel,
// on the transforms, the LDS layout and the strip decomposition of lmc_fft_kernel.h (included by lmc_fft.hip alone, which therefore holds this kernel's
// launcher too).  It is not a further MODE of that kernel: the instantiations of fft_cols_spectral_kernel are a closed list that the resource fence of
// the Fourier-domain data term names one by one.
//
// One workgroup = a strip of `lines` half-plane columns x all H rows of one image, two LDS buffers:
//   1. the strip of nspec (the row transform of the white field) is loaded and column-transformed forward; every lane takes ITS elements of
//      nh sqrt(q) into registers -- element i of a lane is index threadIdx.x + i kFftThreads of the functor loop, H cw = kFftElems for every H, so
//      kFftElems / kFftThreads = 8 complex values per lane;
//   2. barrier; the strip of zspec is loaded, transformed forward, the functor (zh rinv + sf B + regs) / q applied, transformed inverse and stored.
// Two forward column transforms and one inverse through the same two buffers; no pass over HBM for the noise spectrum.  q = sf A + rinv; sqrt and the
// division are IEEE (no fast intrinsic), the products and sums are the fused multiply-adds written below.
#pragma once
#include "lmc_fft_kernel.h"

namespace lmc {

struct SgsColsArgs {
  float2* zspec;         // [n][H][Wh]: the row transform of z, overwritten by the column-inverted spectrum of the draw
  const float2* nspec;   // [n][H][Wh]: the row transform of the white field; NULL: no noise (the conditional mean)
  const float2* tw;      // [kFftTw]
  const float* tab;      // planes A, Re B, Im B, [H][Wh] each
  int H, Wh, logH;
  int lines;             // columns of a strip; a power of two, H lines = kFftElems
  int strips;            // strips of one image
  float rinv, sf;        // 1 / rho^2, sigma_f
};

__global__ __launch_bounds__(kFftThreads) void sgs_cols_gibbs_kernel(SgsColsArgs A) {
  extern __shared__ float2 fft_lds[];
  constexpr int kOwn = kFftElems / kFftThreads;
  static_assert(kOwn * kFftThreads == kFftElems, "a lane owns a whole number of elements");
  const int H = A.H, LS = fft_line_stride(H), cw = A.lines, logcw = __ffs(cw) - 1;
  float2* a = fft_lds;
  float2* b = fft_lds + cw * LS;
  const int64_t img = blockIdx.x / A.strips;
  const int strip = blockIdx.x - (int)(img * A.strips);
  const int c0 = strip * cw, cols = min(cw, A.Wh - c0);
  const size_t off = (size_t)img * H * A.Wh + c0, plane = (size_t)H * A.Wh;
  const float sc = 1.f / sqrtf((float)H);
  float2 nz[kOwn];
#pragma unroll
  for (int i = 0; i < kOwn; ++i) nz[i] = make_float2(0.f, 0.f);
  if (A.nspec) {
    const float2* np = A.nspec + off;
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int t = threadIdx.x + i * kFftThreads, r = t >> logcw, c = t & (cw - 1);
      a[c * LS + fft_slot(r)] = c < cols ? np[(size_t)r * A.Wh + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float2* rn = fft_lines<false>(a, b, A.logH, cw, LS, A.tw);
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int t = threadIdx.x + i * kFftThreads, row = t >> logcw, c = t & (cw - 1);
      if (c < cols) {
        const float2 v = rn[c * LS + fft_slot(row)];
        const float g = sqrtf(fmaf(A.sf, A.tab[(size_t)row * A.Wh + c0 + c], A.rinv));
        nz[i] = make_float2((v.x * sc) * g, (v.y * sc) * g);
      }
    }
    __syncthreads();
  }
  float2* sp = A.zspec + off;
#pragma unroll
  for (int i = 0; i < kOwn; ++i) {
    const int t = threadIdx.x + i * kFftThreads, r = t >> logcw, c = t & (cw - 1);
    a[c * LS + fft_slot(r)] = c < cols ? sp[(size_t)r * A.Wh + c] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  float2* r = fft_lines<false>(a, b, A.logH, cw, LS, A.tw);
#pragma unroll
  for (int i = 0; i < kOwn; ++i) {
    const int t = threadIdx.x + i * kFftThreads, row = t >> logcw, c = t & (cw - 1);
    if (c >= cols) continue;
    const float2 v = r[c * LS + fft_slot(row)];
    const float* p = A.tab + (size_t)row * A.Wh + c0 + c;
    const float q = fmaf(A.sf, p[0], A.rinv);
    r[c * LS + fft_slot(row)] = make_float2(fmaf(v.x * sc, A.rinv, fmaf(A.sf, p[plane], nz[i].x)) / q,
                                            fmaf(v.y * sc, A.rinv, fmaf(A.sf, p[2 * plane], nz[i].y)) / q);
  }
  __syncthreads();
  float2* other = r == a ? b : a;
  const float2* q = fft_lines<true>(r, other, A.logH, cw, LS, A.tw);
#pragma unroll
  for (int i = 0; i < kOwn; ++i) {
    const int t = threadIdx.x + i * kFftThreads, row = t >> logcw, c = t & (cw - 1);
    if (c >= cols) continue;
    const float2 v = q[c * LS + fft_slot(row)];
    sp[(size_t)row * A.Wh + c] = make_float2(v.x * sc, v.y * sc);
  }
}

}  // namespace lmc
