// The spectral data term (LMC_DATA_SPECTRAL, include/lmc_atomi.h): a batched 2-D real FFT that lives in LDS, norm = "ortho", on the half plane of
// Wh = W / 2 + 1 columns, for power-of-two sides 8 .. 1024.
//
//   F: the unitary 2-D DFT of an H x W real image in numpy's unshifted fft2(norm="ortho") index order; G, b: complex H x W, gain and data per frequency.
//   f(x) = sigma_f / 2 sum_k |G_k (F x)_k - b_k|^2 over the full plane,  grad f = sigma_f Re F^H(conj(G) (G F x - b)).
//   x is real, so F x is Hermitian and only the Hermitian part of the residual survives the real part.  With -k = ((-i) mod H, (-j) mod W),
//   A_k = (|G_k|^2 + |G_-k|^2) / 2 (real) and B_k = (conj(G_k) b_k + G_-k conj(b_-k)) / 2:
//     grad f       = sigma_f irfft2(A rfft2(x) - B)                      exactly, on the half plane alone,
//     prox_{t f} v = irfft2((rfft2(v) + t sigma_f B) / (1 + t sigma_f A)),
//     f            = sigma_f / 2 sum over the half plane of |G_k xh_k - b_k|^2 + |conj(G_-k) xh_k - conj(b_-k)|^2, the second term zeroed in the
//                    self-conjugate columns j = 0 and j = W / 2 (where -k is itself visited) -- from the residuals, never the expanded form, which cancels.
//
// One evaluation is three launches: fft_rows_fwd_kernel (real rows -> the Wh columns of the row transform), fft_cols_spectral_kernel (a strip of
// columns x all H rows: forward column transform, a pointwise functor, inverse column transform, in place) and fft_rows_inv_kernel (the Hermitian row
// rebuilt in LDS from its Wh entries, inverted, the real part through an epilogue).  The spectrum buffer is [n][H][Wh] complex, row-major.
//
// The transform is a Stockham autosort between two LDS buffers: radix-4 stages and one radix-2 stage where log2 N is odd.  Twiddles come from ONE table
// of exp(-2 pi i m / 1024), m < 1024, computed in double on the host and rounded once to float32 (every stage of every length up to 1024 indexes it
// with a stride); no fast sine / cosine intrinsic anywhere.  A line of N complex values occupies N + N / 32 + 1 slots: one pad slot after every 32
// values and an odd line stride, so neither the power-of-two strides inside a line nor the stride between lines land on one bank.
#pragma once
#include <hip/hip_runtime.h>

#include "lmc_launch.h"

namespace lmc {

struct FftArgs {
  const float* x;       // rows_fwd: the real images [n][H][W]; rows_inv, kFftOverwrite: x of out = a x - coef v
  float* out;           // rows_inv: the real result [n][H][W]
  float2* spec;         // [n][H][Wh]
  const float2* tw;     // [kFftTw]
  const float* tab;     // functor planes [.][H][Wh]: kFftGrad / kFftProx A, Re B, Im B; kFftMul Re M, Im M; kFftValue planes 3 .. 10 of the descriptor
  double* part;         // kFftValue: [n][strips]
  int64_t rows;         // n * H
  int H, W, Wh, logH, logW;
  int lines;            // lines of one workgroup: rows (row kernels), columns of a strip (column kernel); a power of two
  int strips;           // column kernel: strips of one image
  float a, coef, ts;
};

__device__ __forceinline__ int fft_slot(int i) { return i + (i >> 5); }
__host__ __device__ constexpr int fft_line_stride(int N) { return N + (N >> 5) + 1; }

template <bool INV>
__device__ __forceinline__ float2 fft_twmul(float2 v, float2 w) {      // v w (forward) or v conj(w) (inverse)
  if (INV) return make_float2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y);
  return make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
}

// `lines` transforms of length N = 1 << logN, line l at a + l * LS in fft_slot order; every thread of the workgroup takes part.  Returns the buffer
// that holds the result (a or b), in natural order; ends on a barrier.
template <bool INV>
__device__ float2* fft_lines(float2* a, float2* b, int logN, int lines, int LS, const float2* __restrict__ tw) {
  const int N = 1 << logN;
  int Ns = 1, logNs = 0;
  for (int s = 0; s < (logN >> 1); ++s) {
    const int logq = logN - 2, q = 1 << logq, total = lines << logq;
    const int tstep = kFftTw >> (logNs + 2);
    for (int t = threadIdx.x; t < total; t += kFftThreads) {
      const int line = t >> logq, j = t & (q - 1), k = j & (Ns - 1);
      const float2* src = a + line * LS;
      float2 v0 = src[fft_slot(j)], v1 = src[fft_slot(j + q)], v2 = src[fft_slot(j + 2 * q)], v3 = src[fft_slot(j + 3 * q)];
      if (k) {
        v1 = fft_twmul<INV>(v1, tw[k * tstep]);
        v2 = fft_twmul<INV>(v2, tw[2 * k * tstep]);
        v3 = fft_twmul<INV>(v3, tw[3 * k * tstep]);
      }
      const float2 t0 = make_float2(v0.x + v2.x, v0.y + v2.y), t1 = make_float2(v0.x - v2.x, v0.y - v2.y);
      const float2 t2 = make_float2(v1.x + v3.x, v1.y + v3.y), t3 = make_float2(v1.x - v3.x, v1.y - v3.y);
      const float2 r3 = INV ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x);      // +i t3 (inverse), -i t3 (forward)
      float2* dst = b + line * LS;
      const int j0 = ((j - k) << 2) + k;
      dst[fft_slot(j0)] = make_float2(t0.x + t2.x, t0.y + t2.y);
      dst[fft_slot(j0 + Ns)] = make_float2(t1.x + r3.x, t1.y + r3.y);
      dst[fft_slot(j0 + 2 * Ns)] = make_float2(t0.x - t2.x, t0.y - t2.y);
      dst[fft_slot(j0 + 3 * Ns)] = make_float2(t1.x - r3.x, t1.y - r3.y);
    }
    __syncthreads();
    float2* sw = a; a = b; b = sw;
    Ns <<= 2; logNs += 2;
  }
  if (logN & 1) {
    const int logq = logN - 1, q = 1 << logq, total = lines << logq;
    const int tstep = kFftTw >> (logNs + 1);
    for (int t = threadIdx.x; t < total; t += kFftThreads) {
      const int line = t >> logq, j = t & (q - 1), k = j & (Ns - 1);
      const float2* src = a + line * LS;
      const float2 v0 = src[fft_slot(j)];
      float2 v1 = src[fft_slot(j + q)];
      if (k) v1 = fft_twmul<INV>(v1, tw[k * tstep]);
      float2* dst = b + line * LS;
      const int j0 = ((j - k) << 1) + k;
      dst[fft_slot(j0)] = make_float2(v0.x + v1.x, v0.y + v1.y);
      dst[fft_slot(j0 + Ns)] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    __syncthreads();
    float2* sw = a; a = b; b = sw;
  }
  (void)N;
  return a;
}

// Real rows -> the Wh half-plane columns of their length-W transform, scaled by 1 / sqrt(W).  `lines` rows of the [n * H] rows per workgroup; the last
// workgroup may hold fewer.
__global__ __launch_bounds__(kFftThreads) void fft_rows_fwd_kernel(FftArgs A) {
  extern __shared__ float2 fft_lds[];
  const int W = A.W, LS = fft_line_stride(W);
  float2* a = fft_lds;
  float2* b = fft_lds + A.lines * LS;
  const int64_t r0 = (int64_t)blockIdx.x * A.lines;
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    a[line * LS + fft_slot(i)] = make_float2(row < A.rows ? A.x[row * W + i] : 0.f, 0.f);
  }
  __syncthreads();
  const float2* r = fft_lines<false>(a, b, A.logW, A.lines, LS, A.tw);
  const float sc = 1.f / sqrtf((float)W);
  for (int t = threadIdx.x; t < A.lines * A.Wh; t += kFftThreads) {
    const int line = t / A.Wh, j = t - line * A.Wh;
    const int64_t row = r0 + line;
    if (row >= A.rows) break;
    const float2 v = r[line * LS + fft_slot(j)];
    A.spec[row * A.Wh + j] = make_float2(v.x * sc, v.y * sc);
  }
}

// The Hermitian row rebuilt from its Wh entries, inverted, scaled by 1 / sqrt(W); the real part v goes through the epilogue.
template <int EPI>
__global__ __launch_bounds__(kFftThreads) void fft_rows_inv_kernel(FftArgs A) {
  extern __shared__ float2 fft_lds[];
  const int W = A.W, LS = fft_line_stride(W);
  float2* a = fft_lds;
  float2* b = fft_lds + A.lines * LS;
  const int64_t r0 = (int64_t)blockIdx.x * A.lines;
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    float2 v = make_float2(0.f, 0.f);
    if (row < A.rows) {
      const bool mirror = i > (W >> 1);
      v = A.spec[row * A.Wh + (mirror ? W - i : i)];
      if (mirror) v.y = -v.y;
    }
    a[line * LS + fft_slot(i)] = v;
  }
  __syncthreads();
  const float2* r = fft_lines<true>(a, b, A.logW, A.lines, LS, A.tw);
  const float sc = 1.f / sqrtf((float)W);
  for (int t = threadIdx.x; t < (A.lines << A.logW); t += kFftThreads) {
    const int line = t >> A.logW, i = t & (W - 1);
    const int64_t row = r0 + line;
    if (row >= A.rows) break;
    const float v = r[line * LS + fft_slot(i)].x * sc;
    const int64_t o = row * W + i;
    if (EPI == kFftStore) A.out[o] = v;
    else if (EPI == kFftSub) A.out[o] -= A.coef * v;
    else A.out[o] = A.a * A.x[o] - A.coef * v;
  }
}

// A strip of `lines` half-plane columns x all H rows of one image: forward column transform (1 / sqrt(H)), the functor of MODE, inverse column
// transform (1 / sqrt(H)), written back in place.  kFftColFwd / kFftColInv: one direction and no functor (lmc_rfft2 / lmc_irfft2).  kFftValue: the forward
// transform, then the residuals of the value widened to float64 and summed in a fixed order into part[image][strip]; nothing is written back.
template <int MODE>
__global__ __launch_bounds__(kFftThreads) void fft_cols_spectral_kernel(FftArgs A) {
  extern __shared__ float2 fft_lds[];
  const int H = A.H, LS = fft_line_stride(H), cw = A.lines, logcw = __ffs(cw) - 1;
  float2* a = fft_lds;
  float2* b = fft_lds + cw * LS;
  const int64_t img = blockIdx.x / A.strips;
  const int strip = blockIdx.x - (int)(img * A.strips);
  const int c0 = strip * cw, cols = min(cw, A.Wh - c0);
  float2* sp = A.spec + (size_t)img * H * A.Wh + c0;
  const size_t plane = (size_t)H * A.Wh;
  for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
    const int r = t >> logcw, c = t & (cw - 1);
    a[c * LS + fft_slot(r)] = c < cols ? sp[(size_t)r * A.Wh + c] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const float sc = 1.f / sqrtf((float)H);
  float2* r = a;
  if (MODE != kFftColInv) {
    r = fft_lines<false>(a, b, A.logH, cw, LS, A.tw);
    if (MODE == kFftValue) {
      double acc = 0.0;
      for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
        const int row = t >> logcw, c = t & (cw - 1);
        if (c >= cols) continue;
        float2 v = r[c * LS + fft_slot(row)];
        v.x *= sc; v.y *= sc;
        const float* p = A.tab + (size_t)row * A.Wh + c0 + c;
        const float gr = p[0], gi = p[plane], br = p[2 * plane], bi = p[3 * plane];
        const float hr = p[4 * plane], hi = p[5 * plane], dr = p[6 * plane], di = p[7 * plane];
        const float e0 = gr * v.x - gi * v.y - br, e1 = gr * v.y + gi * v.x - bi;
        const float e2 = hr * v.x - hi * v.y - dr, e3 = hr * v.y + hi * v.x - di;
        acc += (double)e0 * e0 + (double)e1 * e1 + (double)e2 * e2 + (double)e3 * e3;
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
    if (MODE == kFftColFwd) {
      for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
        const int row = t >> logcw, c = t & (cw - 1);
        if (c >= cols) continue;
        const float2 v = r[c * LS + fft_slot(row)];
        sp[(size_t)row * A.Wh + c] = make_float2(v.x * sc, v.y * sc);
      }
      return;
    }
    for (int t = threadIdx.x; t < (H << logcw); t += kFftThreads) {
      const int row = t >> logcw, c = t & (cw - 1);
      if (c >= cols) continue;
      float2 v = r[c * LS + fft_slot(row)];
      v.x *= sc; v.y *= sc;
      const float* p = A.tab + (size_t)row * A.Wh + c0 + c;
      if (MODE == kFftGrad) {
        const float Ak = p[0];
        v = make_float2(Ak * v.x - p[plane], Ak * v.y - p[2 * plane]);
      } else if (MODE == kFftProx) {
        const float d = 1.f / (1.f + A.ts * p[0]);
        v = make_float2((v.x + A.ts * p[plane]) * d, (v.y + A.ts * p[2 * plane]) * d);
      } else {
        const float mr = p[0], mi = p[plane];
        v = make_float2(mr * v.x - mi * v.y, mr * v.y + mi * v.x);
      }
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
    sp[(size_t)row * A.Wh + c] = make_float2(v.x * sc, v.y * sc);
  }
}

__global__ __launch_bounds__(256) void fft_value_finish_kernel(const double* __restrict__ part, int64_t n_img, int strips, double scale,
                                                               double* __restrict__ f_out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_img) return;
  double s = 0.0;
  for (int t = 0; t < strips; ++t) s += part[(size_t)c * strips + t];
  f_out[c] += scale * s;
}

}  // namespace lmc
