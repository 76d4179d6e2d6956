// The multi-coil SENSE data term (LMC_DATA_SENSE, include/lmc_atomi.h): the complex full-plane kernels around fft_lines<INV> of lmc_fft_kernel.h, whose
// transforms, LDS layout (fft_slot, fft_line_stride), twiddle table and 512-thread / kFftElems plan they take as they are (included by lmc_fft.hip alone,
// which therefore holds these kernels' launchers; lmc_sense.hip holds the coil loops).
//
//   x real H x W; S_c complex H x W, c < n_coils; M real H x W, M >= 0; b_c complex H x W; F the unitary 2-D DFT over the full plane.
//   e_c = M F(S_c x) - b_c,   f = sigma_f / 2 sum_c sum_k |e_c,k|^2,   grad f = sigma_f sum_c Re[conj(S_c) F^H(M e_c)].
//
// One coil at a time through one spectrum buffer [n][H][W] complex: sense_rows_fwd_kernel (a row of x times the same row of S_c, transformed, all W
// columns), sense_cols_kernel (a strip of full-plane columns x all H rows: forward column transform, the functor of MODE, inverse column transform) and
// sense_rows_inv_kernel (inverse row transform, times conj(S_c), the real part stored for coil 0 and added for the coils after it).  No atomics; every
// sum has one owner and a fixed order.  The maps and M are read by every chain: plain loads, so that they stay in the caches.
#pragma once
#include "lmc_fft_kernel.h"

namespace lmc {

struct SenseArgs {
  const float* x;          // rows_fwd: the real images [n][H][W]
  float* out;              // rows_inv: the real result [n][H][W]
  const float2* src;       // cols: the spectra read, image i at src + i * src_stride
  float2* spec;            // rows_fwd / cols: the spectra written, image i at spec + i * spec_stride; rows_inv: the spectra read
  const float2* tw;        // [kFftTw]
  const float* s;          // rows kernels: Re S_c [H][W], Im S_c one plane after it
  const float* m;          // cols: M [H][W]
  const float* b;          // cols, kSenseGrad / kSenseValue: Re b_c [H][W], Im b_c one plane after it
  double* part;            // kSenseValue: [n][strips]
  int64_t rows;            // n * H
  int64_t src_stride, spec_stride;      // complex values between the images
  int H, W, logH, logW;
  int lines;               // lines of one workgroup: rows (row kernels), columns of a strip (column kernel); a power of two
  int strips;              // column kernel: strips of one image
};

// x S_c, row by row -> all W columns of the length-W transform, scaled by 1 / sqrt(W).  `lines` rows of the [n * H] rows per workgroup; the last workgroup may
// hold fewer.
__global__ __launch_bounds__(kFftThreads) void sense_rows_fwd_kernel(SenseArgs A) {
  extern __shared__ float2 fft_lds[];
  const int W = A.W, LS = fft_line_stride(W);
  const size_t plane = (size_t)A.H * W;
  float2* a = fft_lds;
  float2* b = fft_lds + A.lines * LS;
  const int64_t r0 = (int64_t)blockIdx.x * A.lines;
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    float2 v = make_float2(0.f, 0.f);
    if (row < A.rows) {
      const float xv = A.x[row * W + i];
      const size_t p = (size_t)(row & (A.H - 1)) * W + i;
      v = make_float2(A.s[p] * xv, A.s[plane + p] * xv);
    }
    a[line * LS + fft_slot(i)] = v;
  }
  __syncthreads();
  const float2* r = fft_lines<false>(a, b, A.logW, A.lines, LS, A.tw);
  const float sc = 1.f / sqrtf((float)W);
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, j = t & (W - 1);
    const int64_t row = r0 + line;
    if (row >= A.rows) break;
    const float2 v = r[line * LS + fft_slot(j)];
    A.spec[(size_t)(row >> A.logH) * A.spec_stride + (size_t)(row & (A.H - 1)) * W + j] = make_float2(v.x * sc, v.y * sc);
  }
}

// The inverse row transform of all W columns, scaled by 1 / sqrt(W); v = Re[conj(S_c) .] goes through the epilogue.  The spectra are dense ([n][H][W]).
template <int EPI>
__global__ __launch_bounds__(kFftThreads) void sense_rows_inv_kernel(SenseArgs A) {
  extern __shared__ float2 fft_lds[];
  const int W = A.W, LS = fft_line_stride(W);
  const size_t plane = (size_t)A.H * W;
  float2* a = fft_lds;
  float2* b = fft_lds + A.lines * LS;
  const int64_t r0 = (int64_t)blockIdx.x * A.lines;
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    a[line * LS + fft_slot(i)] = row < A.rows ? A.spec[row * W + i] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const float2* r = fft_lines<true>(a, b, A.logW, A.lines, LS, A.tw);
  const float sc = 1.f / sqrtf((float)W);
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    if (row >= A.rows) break;
    const float2 u = r[line * LS + fft_slot(i)];
    const size_t p = (size_t)(row & (A.H - 1)) * W + i;
    const float v = (A.s[p] * u.x + A.s[plane + p] * u.y) * sc;
    const int64_t o = row * W + i;
    if (EPI == kSenseStore) A.out[o] = v;
    else A.out[o] += v;
  }
}

// A strip of `lines` full-plane columns x all H rows of one image, read from src and written to spec (the same array where the pass runs in place); a
// partial last strip where W is no multiple of `lines`.  kSenseGrad: forward column transform (1 / sqrt(H)), v <- M (M v - b_c), inverse column transform
// (1 / sqrt(H)).  kSenseValue: the forward transform, then |M v - b_c|^2 from the fp32 residual, widened to float64 and summed in a fixed order into
// part[image][strip]; nothing is written back.  kSenseFwd: the forward transform, v <- M v (the operator).  kSenseAdj: v <- M v, the inverse transform
// (its adjoint).
template <int MODE>
__global__ __launch_bounds__(kFftThreads) void sense_cols_kernel(SenseArgs A) {
  extern __shared__ float2 fft_lds[];
  const int H = A.H, W = A.W, LS = fft_line_stride(H), cw = A.lines, logcw = __ffs(cw) - 1;
  float2* a = fft_lds;
  float2* b = fft_lds + cw * LS;
  const int64_t img = blockIdx.x / A.strips;
  const int strip = blockIdx.x - (int)(img * A.strips);
  const int c0 = strip * cw, cols = min(cw, W - c0);
  const float2* sp = A.src + (size_t)img * A.src_stride + c0;
  float2* dp = A.spec + (size_t)img * A.spec_stride + c0;
  const size_t plane = (size_t)H * W;
  const float sc = 1.f / sqrtf((float)H);
  for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
    const int r = t >> logcw, c = t & (cw - 1);
    float2 v = make_float2(0.f, 0.f);
    if (c < cols) {
      v = sp[(size_t)r * W + c];
      if (MODE == kSenseAdj) {
        const float mk = A.m[(size_t)r * W + c0 + c];
        v.x *= mk; v.y *= mk;
      }
    }
    a[c * LS + fft_slot(r)] = v;
  }
  __syncthreads();
  float2* r = a;
  if (MODE != kSenseAdj) {
    r = fft_lines<false>(a, b, A.logH, cw, LS, A.tw);
    if (MODE == kSenseValue) {
      double acc = 0.0;
      for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
        const int row = t >> logcw, c = t & (cw - 1);
        if (c >= cols) continue;
        const float2 v = r[c * LS + fft_slot(row)];
        const size_t p = (size_t)row * W + c0 + c;
        const float mk = A.m[p];
        const float e0 = mk * (v.x * sc) - A.b[p], e1 = mk * (v.y * sc) - A.b[plane + p];
        acc += (double)e0 * e0 + (double)e1 * e1;
      }
      __syncthreads();
      double* red = reinterpret_cast<double*>(fft_lds);
      red[threadIdx.x] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < kFftThreads; ++i) s += red[i];
        A.part[(size_t)img * A.strips + strip] = s;
      }
      return;
    }
    if (MODE == kSenseFwd) {
      for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
        const int row = t >> logcw, c = t & (cw - 1);
        if (c >= cols) continue;
        const float2 v = r[c * LS + fft_slot(row)];
        const float mk = A.m[(size_t)row * W + c0 + c];
        dp[(size_t)row * W + c] = make_float2(mk * (v.x * sc), mk * (v.y * sc));
      }
      return;
    }
    for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
      const int row = t >> logcw, c = t & (cw - 1);
      if (c >= cols) continue;
      float2 v = r[c * LS + fft_slot(row)];
      const size_t p = (size_t)row * W + c0 + c;
      const float mk = A.m[p];
      v = make_float2(mk * (mk * (v.x * sc) - A.b[p]), mk * (mk * (v.y * sc) - A.b[plane + p]));
      r[c * LS + fft_slot(row)] = v;
    }
    __syncthreads();
  }
  float2* other = r == a ? b : a;
  const float2* q = fft_lines<true>(r, other, A.logH, cw, LS, A.tw);
  for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
    const int row = t >> logcw, c = t & (cw - 1);
    if (c >= cols) continue;
    const float2 v = q[c * LS + fft_slot(row)];
    dp[(size_t)row * W + c] = make_float2(v.x * sc, v.y * sc);
  }
}

// Step 3 of the update: out -= coef g, or (ALONE, without prox and noise) out = a x - coef g.  Elementwise over n floats.
template <bool ALONE>
__global__ __launch_bounds__(256) void sense_axpy_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ out, size_t n, float a,
                                                         float coef) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (ALONE) out[i] = a * x[i] - coef * g[i];
    else out[i] -= coef * g[i];
  }
}

}  // namespace lmc
