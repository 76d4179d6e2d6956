// Daubechies wavelet-l1 prior (LMC_PRIOR_WAVELET_L1; include/lmc_atomi.h is the definition): the multi-level periodic 2-D transform W of the
// extremal-phase filters db1 .. db4, its transpose, the prox W^T soft(W x, thr) and the value sigma sum |details|.
//   wav_fwd_kernel   one level of W.  A workgroup owns kTH x kTW coefficients of each of the four subbands of one image: it stages the
//                    (2 kTH + 2p - 2) x (2 kTW + 2p - 2) input pixels in LDS (the periodic wrap is resolved by the loads: every level wraps at most
//                    once), filters along the rows, then along the columns, and stores LL to the ping-pong buffer of the next level and the three
//                    detail subbands to their Mallat quadrants -- as they are (W alone), soft-thresholded (prox), or not at all (value: their
//                    absolute values are summed in float64, one partial sum per workgroup in a slot of its own).
//   wav_inv_kernel   one level of W^T, the mirror image: four subband tiles with a halo of p - 1 coefficients above and to the left in LDS, the
//                    synthesis along the columns, then along the rows, a 2 kTH x 2 kTW tile of the finer approximation out.
//   wav_value_sum    val[i] = sigma * (the partial sums of image i in slot order): no atomics, two runs give the same bits.
// The taps are template arguments (immediates); LDS rows are read 16 bytes per lane; global loads and stores are 16 bytes per lane where the
// sub-image is aligned for it (row length and stride multiples of 4) and 4 bytes per lane, still consecutive, elsewhere.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

namespace {

constexpr int kTH = 16, kTW = 64;      // coefficients per subband and workgroup

// Daubechies extremal-phase scaling filters (spectral factorisation, sum = sqrt 2) in float64; tests/test_wavelet_reference.py holds them against
// the factorisation itself.  A function with a local table, so that a tap whose index is known after unrolling folds to an immediate.
template <int P>
__host__ __device__ constexpr double db_tap(int k) {
  static_assert(P >= 1 && P <= 4, "db1 .. db4");
  if (P == 1) { constexpr double t[8] = {0.7071067811865476, 0.7071067811865476}; return t[k]; }
  if (P == 2) { constexpr double t[8] = {0.48296291314453416, 0.8365163037378078, 0.2241438680420134, -0.12940952255126037}; return t[k]; }
  if (P == 3) {
    constexpr double t[8] = {0.3326705529500826, 0.8068915093110924, 0.4598775021184915, -0.1350110200102546, -0.08544127388202669, 0.035226291885709526};
    return t[k];
  }
  constexpr double t[8] = {0.2303778133088965, 0.7148465705529157, 0.630880767929859, -0.027983769416859698, -0.1870348117190931, 0.030841381835560653,
                           0.032883011666885176, -0.010597401785069025};
  return t[k];
}
// scaling tap h[k] and wavelet tap g[k] = (-1)^k h[2p - 1 - k], as floats
template <int P> __host__ __device__ constexpr float tap_h(int k) { return (float)db_tap<P>(k); }
template <int P> __host__ __device__ constexpr float tap_g(int k) { return (float)((k & 1) ? -db_tap<P>(2 * P - 1 - k) : db_tap<P>(2 * P - 1 - k)); }

__device__ __forceinline__ float soft_thr(float v, float t) { return copysignf(fmaxf(fabsf(v) - t, 0.f), v); }

// One level, both directions.  fine: the n_r x n_c image of the finer scale (forward: read; inverse: written).  ll: the (n_r / 2) x (n_c / 2)
// approximation of the coarser scale (forward: written; inverse: read), with a row and image stride of its own (compact ping-pong buffer, or the corner
// of the pyramid for the last level).  det: the pyramid, whose n_r x n_c corner holds the three detail subbands of this level in its other quadrants --
// filtered g along the rows: to the right; along the columns: below.
struct WavLevel {
  const float* fine_in;  float* fine_out;  int fine_stride;  size_t fine_img;
  const float* ll_in;    float* ll_out;    int ll_stride;    size_t ll_img;
  const float* det_in;   float* det_out;   int det_stride;   size_t det_img;      // Mallat pyramid: the quadrants of its n_r x n_c corner
  int n_r, n_c;
  int tiles_x, tiles;                  // tiles per image row of tiles, per image
  int vec_fine, vec_ll, vec_det;       // 16-byte accesses are aligned on that array
  float thr;
  double* part;  int part_stride, part_off;      // value: part[image * part_stride + part_off + tile]
};

enum { kWavRaw = 0, kWavSoft = 1, kWavValue = 2 };

template <int P, int MODE>
__global__ __launch_bounds__(256) void wav_fwd_kernel(WavLevel L) {
  constexpr int RI = 2 * kTH + 2 * P - 2;       // input rows of a tile
  constexpr int TWI = 2 * kTW + 8;              // input columns, padded to what the row pass reads (whole float4s)
  constexpr int RW = 2 * kTW;                   // row-pass output: lo in columns [0, kTW), hi in [kTW, 2 kTW)
  __shared__ __attribute__((aligned(16))) float T[RI * TWI];
  __shared__ __attribute__((aligned(16))) float R[RI * RW];
  __shared__ double red[256 / kWave];
  const int tid = threadIdx.x;
  const size_t im = blockIdx.x / (unsigned)L.tiles;
  const int tile = blockIdx.x - (unsigned)im * (unsigned)L.tiles;
  const int hr = L.n_r >> 1, hc = L.n_c >> 1;
  const int r0 = (tile / L.tiles_x) * kTH, c0 = (tile % L.tiles_x) * kTW;      // first coefficient of the tile
  const int th = min(kTH, hr - r0), tw = min(kTW, hc - c0);
  const int rows_in = 2 * th + 2 * P - 2, cols_in = 2 * tw + 2 * P - 2;
  const float* __restrict__ src = L.fine_in + im * L.fine_img;

  // ---- stage the input tile, wrap resolved here
  if (L.vec_fine) {
    const int g4 = (cols_in + 3) >> 2;
    for (int e = tid; e < rows_in * g4; e += 256) {
      const int r = e / g4, g = e - r * g4;
      int gr = 2 * r0 + r, gc = 2 * c0 + 4 * g;
      if (gr >= L.n_r) gr -= L.n_r;
      if (gc >= L.n_c) gc -= L.n_c;
      *reinterpret_cast<float4*>(&T[r * TWI + 4 * g]) = *reinterpret_cast<const float4*>(src + (size_t)gr * L.fine_stride + gc);
    }
  } else {
    for (int e = tid; e < rows_in * cols_in; e += 256) {
      const int r = e / cols_in, c = e - r * cols_in;
      int gr = 2 * r0 + r, gc = 2 * c0 + c;
      if (gr >= L.n_r) gr -= L.n_r;
      if (gc >= L.n_c) gc -= L.n_c;
      T[r * TWI + c] = src[(size_t)gr * L.fine_stride + gc];
    }
  }
  __syncthreads();

  // ---- along the rows: a lane forms coefficients 2q and 2q + 1 of both bands from 2p + 2 pixels, read as float4s
  {
    constexpr int NV = (2 * P + 2 + 3) / 4;
    const int nq = (tw + 1) >> 1;
    for (int e = tid; e < rows_in * nq; e += 256) {
      const int r = e / nq, q = e - r * nq;
      float v[4 * NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(&T[r * TWI + 4 * q + 4 * i]);
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
      }
      float lo0 = 0.f, lo1 = 0.f, hi0 = 0.f, hi1 = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * P; ++k) {
        lo0 = fmaf(tap_h<P>(k), v[k], lo0);
        hi0 = fmaf(tap_g<P>(k), v[k], hi0);
        lo1 = fmaf(tap_h<P>(k), v[k + 2], lo1);
        hi1 = fmaf(tap_g<P>(k), v[k + 2], hi1);
      }
      *reinterpret_cast<float2*>(&R[r * RW + 2 * q]) = make_float2(lo0, lo1);
      *reinterpret_cast<float2*>(&R[r * RW + kTW + 2 * q]) = make_float2(hi0, hi1);
    }
  }
  __syncthreads();

  // ---- along the columns: a lane forms four neighbouring coefficients of a row of both bands
  double acc = 0.0;
  {
    constexpr int G = RW / 4;
    for (int e = tid; e < th * G; e += 256) {
      const int mr = e / G, g = e - mr * G;
      const int cb = 4 * g;                          // column in R
      const bool rhi = cb >= kTW;                    // the row band of these four
      const int cc = rhi ? cb - kTW : cb;            // coefficient column inside the tile
      if (cc >= tw) continue;
      float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2 * P; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(&R[(2 * mr + k) * RW + cb]);
        lo[0] = fmaf(tap_h<P>(k), t.x, lo[0]); lo[1] = fmaf(tap_h<P>(k), t.y, lo[1]);
        lo[2] = fmaf(tap_h<P>(k), t.z, lo[2]); lo[3] = fmaf(tap_h<P>(k), t.w, lo[3]);
        hi[0] = fmaf(tap_g<P>(k), t.x, hi[0]); hi[1] = fmaf(tap_g<P>(k), t.y, hi[1]);
        hi[2] = fmaf(tap_g<P>(k), t.z, hi[2]); hi[3] = fmaf(tap_g<P>(k), t.w, hi[3]);
      }
      const int nv = min(4, tw - cc);                // valid ones of the four
      const int gr = r0 + mr, gc = c0 + cc;
      // columns-lo of rows-lo is LL; the other three are details
      float* dlo = nullptr; float* dhi;
      bool vlo = false, vhi = L.vec_det != 0;
      if (!rhi) {
        dlo = L.ll_out + im * L.ll_img + (size_t)gr * L.ll_stride + gc;
        vlo = L.vec_ll != 0;
        dhi = MODE == kWavValue ? nullptr : L.det_out + im * L.det_img + (size_t)(hr + gr) * L.det_stride + gc;
      } else {
        if (MODE != kWavValue) dlo = L.det_out + im * L.det_img + (size_t)gr * L.det_stride + hc + gc;
        vlo = L.vec_det != 0;
        dhi = MODE == kWavValue ? nullptr : L.det_out + im * L.det_img + (size_t)(hr + gr) * L.det_stride + hc + gc;
      }
      if (MODE == kWavSoft) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { hi[i] = soft_thr(hi[i], L.thr); if (rhi) lo[i] = soft_thr(lo[i], L.thr); }
      }
      if (MODE == kWavValue) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < nv) s += fabsf(hi[i]) + (rhi ? fabsf(lo[i]) : 0.f);
        acc += (double)s;
      }
      if (dlo) {
        if (vlo && nv == 4) *reinterpret_cast<float4*>(dlo) = make_float4(lo[0], lo[1], lo[2], lo[3]);
        else {
#pragma unroll
          for (int i = 0; i < 4; ++i) if (i < nv) dlo[i] = lo[i];
        }
      }
      if (dhi) {
        if (vhi && nv == 4) *reinterpret_cast<float4*>(dhi) = make_float4(hi[0], hi[1], hi[2], hi[3]);
        else {
#pragma unroll
          for (int i = 0; i < 4; ++i) if (i < nv) dhi[i] = hi[i];
        }
      }
    }
  }
  if (MODE == kWavValue) {
    const double tot = block_sum(acc, red);
    if (tid == 0) L.part[im * (size_t)L.part_stride + L.part_off + tile] = tot;
  }
}

template <int P>
__global__ __launch_bounds__(256) void wav_inv_kernel(WavLevel L) {
  constexpr int HR = kTH + P - 1;               // subband rows of a tile with the halo above
  constexpr int SW = kTW + 4;                   // subband columns: a whole float4 of halo to the left (p - 1 <= 3 of it used)
  constexpr int G = SW / 4;
  __shared__ __attribute__((aligned(16))) float S[4 * HR * SW];       // ll, hl (rows-hi, columns-lo), lh (rows-lo, columns-hi), hh
  __shared__ __attribute__((aligned(16))) float Y[2 * 2 * kTH * SW];  // after the column synthesis: rows-lo band, rows-hi band
  const int tid = threadIdx.x;
  const size_t im = blockIdx.x / (unsigned)L.tiles;
  const int tile = blockIdx.x - (unsigned)im * (unsigned)L.tiles;
  const int hr = L.n_r >> 1, hc = L.n_c >> 1;
  const int r0 = (tile / L.tiles_x) * kTH, c0 = (tile % L.tiles_x) * kTW;
  const int th = min(kTH, hr - r0), tw = min(kTW, hc - c0);
  const float* __restrict__ ll = L.ll_in + im * L.ll_img;
  const float* __restrict__ det = L.det_in + im * L.det_img;

  // ---- stage the four subband tiles; S row i = subband row r0 - (P - 1) + i, S column j = subband column c0 - 4 + j (both wrapped)
  const int rows_in = th + P - 1;
  for (int b = 0; b < 4; ++b) {
    // b & 1: rows-hi (columns offset hc in the pyramid), b & 2: columns-hi (rows offset hr)
    const bool is_ll = b == 0;
    const float* __restrict__ base = is_ll ? ll : det + (size_t)((b & 2) ? hr : 0) * L.det_stride + ((b & 1) ? hc : 0);
    const int stride = is_ll ? L.ll_stride : L.det_stride;
    const bool vec = (is_ll ? L.vec_ll : L.vec_det) != 0;
    float* __restrict__ Sb = S + b * HR * SW;
    if (vec) {
      const int g4 = 1 + ((tw + 3) >> 2);
      for (int e = tid; e < rows_in * g4; e += 256) {
        const int r = e / g4, g = e - r * g4;
        int gr = r0 - (P - 1) + r, gc = c0 - 4 + 4 * g;
        if (gr < 0) gr += hr;
        if (gc < 0) gc += hc;
        *reinterpret_cast<float4*>(&Sb[r * SW + 4 * g]) = *reinterpret_cast<const float4*>(base + (size_t)gr * stride + gc);
      }
    } else {
      const int cols_in = tw + P - 1;
      for (int e = tid; e < rows_in * cols_in; e += 256) {
        const int r = e / cols_in, c = e - r * cols_in;
        int gr = r0 - (P - 1) + r, gc = c0 - (P - 1) + c;
        if (gr < 0) gr += hr;
        if (gc < 0) gc += hc;
        Sb[r * SW + 4 - (P - 1) + c] = base[(size_t)gr * stride + gc];
      }
    }
  }
  __syncthreads();

  // ---- along the columns: rows 2j and 2j + 1 of the row band sb from its columns-lo and columns-hi subbands, four columns per lane
  for (int e = tid; e < 2 * th * G; e += 256) {
    const int sb = e / (th * G), rem = e - sb * (th * G);
    const int j = rem / G, g = rem - j * G;
    const float* __restrict__ Slo = S + sb * HR * SW;              // columns-lo: ll (sb 0) or the rows-hi subband (sb 1)
    const float* __restrict__ Shi = S + (2 + sb) * HR * SW;        // columns-hi
    float y0[4] = {0.f, 0.f, 0.f, 0.f}, y1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(&Slo[(j + (P - 1) - q) * SW + 4 * g]);
      const float4 d = *reinterpret_cast<const float4*>(&Shi[(j + (P - 1) - q) * SW + 4 * g]);
      const float av[4] = {a.x, a.y, a.z, a.w}, dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        y0[i] = fmaf(tap_h<P>(2 * q), av[i], y0[i]);     y0[i] = fmaf(tap_g<P>(2 * q), dv[i], y0[i]);
        y1[i] = fmaf(tap_h<P>(2 * q + 1), av[i], y1[i]); y1[i] = fmaf(tap_g<P>(2 * q + 1), dv[i], y1[i]);
      }
    }
    float* __restrict__ Yb = Y + sb * 2 * kTH * SW;
    *reinterpret_cast<float4*>(&Yb[(2 * j) * SW + 4 * g]) = make_float4(y0[0], y0[1], y0[2], y0[3]);
    *reinterpret_cast<float4*>(&Yb[(2 * j + 1) * SW + 4 * g]) = make_float4(y1[0], y1[1], y1[2], y1[3]);
  }
  __syncthreads();

  // ---- along the rows: eight neighbouring pixels of a row per lane (subband columns 4u .. 4u + 3), from two float4s of each band
  float* __restrict__ dst = L.fine_out + im * L.fine_img;
  constexpr int U = kTW / 4;
  for (int e = tid; e < 2 * th * U; e += 256) {
    const int i = e / U, u = e - i * U;
    if (4 * u >= tw) continue;
    const float* __restrict__ Ylo = Y + i * SW + 4 * u;            // Y columns 4u .. 4u + 7 = subband columns 4u - 4 .. 4u + 3
    const float* __restrict__ Yhi = Y + 2 * kTH * SW + i * SW + 4 * u;
    const float4 a0 = *reinterpret_cast<const float4*>(Ylo), a1 = *reinterpret_cast<const float4*>(Ylo + 4);
    const float4 d0 = *reinterpret_cast<const float4*>(Yhi), d1 = *reinterpret_cast<const float4*>(Yhi + 4);
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    float o[8];
#pragma unroll
    for (int jc = 0; jc < 4; ++jc) {
      float e0 = 0.f, e1 = 0.f;
#pragma unroll
      for (int q = 0; q < P; ++q) {
        e0 = fmaf(tap_h<P>(2 * q), av[4 + jc - q], e0);     e0 = fmaf(tap_g<P>(2 * q), dv[4 + jc - q], e0);
        e1 = fmaf(tap_h<P>(2 * q + 1), av[4 + jc - q], e1); e1 = fmaf(tap_g<P>(2 * q + 1), dv[4 + jc - q], e1);
      }
      o[2 * jc] = e0; o[2 * jc + 1] = e1;
    }
    const int nv = 2 * min(4, tw - 4 * u);         // valid pixels of the eight
    float* p = dst + (size_t)(2 * r0 + i) * L.fine_stride + 2 * c0 + 8 * u;
    if (L.vec_fine && nv == 8) {
      *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<float4*>(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) if (k < nv) p[k] = o[k];
    }
  }
}

__global__ __launch_bounds__(256) void wav_value_sum_kernel(const double* __restrict__ part, int64_t n_img, int n_part, float sigma, double* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_img) return;
  double a = 0.0;
  for (int k = 0; k < n_part; ++k) a += part[(size_t)i * n_part + k];
  val[i] = (double)sigma * a;
}

inline int tiles_of(int n_r, int n_c, int* tx) {
  const int x = ((n_c >> 1) + kTW - 1) / kTW, y = ((n_r >> 1) + kTH - 1) / kTH;
  if (tx) *tx = x;
  return x * y;
}

inline int aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int vec_ok(const void* p, int cols, int stride, size_t img) { return aligned16(p) && (cols & 3) == 0 && (stride & 3) == 0 && (img & 3) == 0; }

// the images of a level in launches of at most 2^30 workgroups
template <class K>
hipError_t launch_level(K kernel, WavLevel L, int64_t n_img, hipStream_t st) {
  const int64_t chunk = ((int64_t)1 << 30) / L.tiles;
  for (int64_t i0 = 0; i0 < n_img; i0 += chunk) {
    const int64_t n = (n_img - i0) < chunk ? (n_img - i0) : chunk;
    WavLevel C = L;
    if (C.fine_in) C.fine_in += i0 * L.fine_img;
    if (C.fine_out) C.fine_out += i0 * L.fine_img;
    if (C.ll_in) C.ll_in += i0 * L.ll_img;
    if (C.ll_out) C.ll_out += i0 * L.ll_img;
    if (C.det_in) C.det_in += i0 * L.det_img;
    if (C.det_out) C.det_out += i0 * L.det_img;
    if (C.part) C.part += i0 * L.part_stride;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n * L.tiles)), dim3(256), 0, st, C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <int P>
hipError_t fwd_level(int mode, const WavLevel& L, int64_t n_img, hipStream_t st) {
  switch (mode) {
    case kWavRaw: return launch_level(wav_fwd_kernel<P, kWavRaw>, L, n_img, st);
    case kWavSoft: return launch_level(wav_fwd_kernel<P, kWavSoft>, L, n_img, st);
    default: return launch_level(wav_fwd_kernel<P, kWavValue>, L, n_img, st);
  }
}

hipError_t fwd_level(int p, int mode, const WavLevel& L, int64_t n_img, hipStream_t st) {
  switch (p) {
    case 1: return fwd_level<1>(mode, L, n_img, st);
    case 2: return fwd_level<2>(mode, L, n_img, st);
    case 3: return fwd_level<3>(mode, L, n_img, st);
    case 4: return fwd_level<4>(mode, L, n_img, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t inv_level(int p, const WavLevel& L, int64_t n_img, hipStream_t st) {
  switch (p) {
    case 1: return launch_level(wav_inv_kernel<1>, L, n_img, st);
    case 2: return launch_level(wav_inv_kernel<2>, L, n_img, st);
    case 3: return launch_level(wav_inv_kernel<3>, L, n_img, st);
    case 4: return launch_level(wav_inv_kernel<4>, L, n_img, st);
    default: return hipErrorInvalidValue;
  }
}

// The approximation of level j (1 .. levels - 1) lives compact, (H >> j) x (W >> j) per image, in `odd` (j odd) or `even` (j even); that of the
// last level in the corner of the pyramid.
struct LLHome { float* p; int stride; size_t img; };
LLHome ll_home(int j, int levels, int H, int W, float* odd, float* even, float* pyr) {
  if (j == levels) return {pyr, W, (size_t)H * W};
  return {(j & 1) ? odd : even, W >> j, (size_t)(H >> j) * (W >> j)};
}

// W (mode kWavRaw / kWavSoft: details into pyr) or the value (kWavValue: pyr unused, partial sums into part)
hipError_t forward(const float* x, int64_t n_img, int H, int W, int p, int levels, int mode, float thr, float* pyr, float* odd, float* even, double* part,
                   int part_stride, hipStream_t st) {
  int off = 0;
  for (int j = 1; j <= levels; ++j) {
    WavLevel L{};
    L.n_r = H >> (j - 1); L.n_c = W >> (j - 1);
    if (j == 1) { L.fine_in = x; L.fine_stride = W; L.fine_img = (size_t)H * W; }
    else { const LLHome h = ll_home(j - 1, levels, H, W, odd, even, pyr); L.fine_in = h.p; L.fine_stride = h.stride; L.fine_img = h.img; }
    // value: the last approximation is not needed, but the kernel has one form: it goes to the buffer of its parity like the others
    const LLHome o = ll_home(j, mode == kWavValue ? levels + 1 : levels, H, W, odd, even, pyr);
    L.ll_out = o.p; L.ll_stride = o.stride; L.ll_img = o.img;
    L.det_out = pyr; L.det_stride = W; L.det_img = (size_t)H * W;
    L.tiles = tiles_of(L.n_r, L.n_c, &L.tiles_x);
    L.vec_fine = vec_ok(L.fine_in, L.n_c, L.fine_stride, L.fine_img);
    L.vec_ll = vec_ok(L.ll_out, L.n_c >> 1, L.ll_stride, L.ll_img);
    L.vec_det = mode == kWavValue ? 0 : vec_ok(pyr, L.n_c >> 1, W, L.det_img);
    L.thr = thr;
    L.part = part; L.part_stride = part_stride; L.part_off = off;
    off += L.tiles;
    const hipError_t e = fwd_level(p, mode, L, n_img, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// W^T of the pyramid pyr into out
hipError_t inverse(const float* pyr, float* out, int64_t n_img, int H, int W, int p, int levels, float* odd, float* even, hipStream_t st) {
  for (int j = levels; j >= 1; --j) {
    WavLevel L{};
    L.n_r = H >> (j - 1); L.n_c = W >> (j - 1);
    const LLHome h = ll_home(j, levels, H, W, odd, even, const_cast<float*>(pyr));
    L.ll_in = h.p; L.ll_stride = h.stride; L.ll_img = h.img;
    L.det_in = pyr; L.det_stride = W; L.det_img = (size_t)H * W;
    if (j == 1) { L.fine_out = out; L.fine_stride = W; L.fine_img = (size_t)H * W; }
    else { const LLHome o = ll_home(j - 1, levels, H, W, odd, even, nullptr); L.fine_out = o.p; L.fine_stride = o.stride; L.fine_img = o.img; }
    L.tiles = tiles_of(L.n_r, L.n_c, &L.tiles_x);
    L.vec_fine = vec_ok(L.fine_out, L.n_c, L.fine_stride, L.fine_img);
    L.vec_ll = vec_ok(L.ll_in, L.n_c >> 1, L.ll_stride, L.ll_img);
    L.vec_det = vec_ok(pyr, L.n_c >> 1, W, L.det_img);
    const hipError_t e = inv_level(p, L, n_img, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

bool wavelet_shape_ok(int H, int W, int p, int levels) {
  if (p < 1 || p > kWaveletMaxP || levels < 1 || levels > LMC_MAX_WAVELET_LEVELS || H < 1 || W < 1) return false;
  const int m = (1 << levels) - 1;
  if ((H & m) || (W & m)) return false;
  return ((H < W ? H : W) >> (levels - 1)) >= 2 * p;
}

int wavelet_filter(int p, double* h) {
  switch (p) {
    case 1: for (int k = 0; k < 2; ++k) h[k] = db_tap<1>(k); return 2;
    case 2: for (int k = 0; k < 4; ++k) h[k] = db_tap<2>(k); return 4;
    case 3: for (int k = 0; k < 6; ++k) h[k] = db_tap<3>(k); return 6;
    case 4: for (int k = 0; k < 8; ++k) h[k] = db_tap<4>(k); return 8;
    default: return 0;
  }
}

size_t wavelet_ll_floats(int64_t n_img, int H, int W) { return (size_t)n_img * (size_t)(H >> 1) * (size_t)(W >> 1); }
size_t wavelet_ws_floats(int64_t n_img, int H, int W) { return (size_t)n_img * H * W + wavelet_ll_floats(n_img, H, W); }

int wavelet_partials(int H, int W, int levels) {
  int n = 0;
  for (int j = 1; j <= levels; ++j) n += tiles_of(H >> (j - 1), W >> (j - 1), nullptr);
  return n;
}

hipError_t launch_wavelet_prox(const float* x, float* out, int64_t n_img, int H, int W, int p, int levels, float thr, float* ws, hipStream_t st) {
  if (!x || !out || !ws || x == out || n_img < 1 || !wavelet_shape_ok(H, W, p, levels)) return hipErrorInvalidValue;
  float* pyr = ws;
  float* odd = ws + (size_t)n_img * H * W;
  // approximations of even levels pass through `out`: it is free until the last inverse level writes it, and that level reads level 1 from `odd`
  hipError_t e = forward(x, n_img, H, W, p, levels, kWavSoft, thr, pyr, odd, out, nullptr, 0, st);
  if (e != hipSuccess) return e;
  return inverse(pyr, out, n_img, H, W, p, levels, odd, out, st);
}

hipError_t launch_wavelet_value(const float* x, int64_t n_img, int H, int W, int p, int levels, float sigma, float* ws, double* part, double* val,
                                hipStream_t st) {
  if (!x || !val || !ws || !part || n_img < 1 || !wavelet_shape_ok(H, W, p, levels)) return hipErrorInvalidValue;
  const int np = wavelet_partials(H, W, levels);
  float* odd = ws;
  float* even = ws + wavelet_ll_floats(n_img, H, W);      // (a quarter of `odd` is used)
  hipError_t e = forward(x, n_img, H, W, p, levels, kWavValue, 0.f, nullptr, odd, even, part, np, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wav_value_sum_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, n_img, np, sigma, val);
  return hipGetLastError();
}

hipError_t launch_wavelet_apply(const float* x, float* out, int64_t n_img, int H, int W, int p, int levels, int inverse_dir, float* ws, hipStream_t st) {
  if (!x || !out || !ws || x == out || n_img < 1 || !wavelet_shape_ok(H, W, p, levels)) return hipErrorInvalidValue;
  float* odd = ws;
  float* even = ws + wavelet_ll_floats(n_img, H, W);
  if (inverse_dir) return inverse(x, out, n_img, H, W, p, levels, odd, even, st);
  return forward(x, n_img, H, W, p, levels, kWavRaw, 0.f, out, odd, even, nullptr, 0, st);
}

}  // namespace lmc
