// The parallel-beam Radon operator (LMC_DATA_RADON .. LMC_DATA_HUBER_RADON, lmc_radon_apply): the pixel-driven projector with linear interpolation on
// the detector; include/lmc_atomi.h holds the definition.  Pixel (i, j) meets the detector of angle a at t = ax[a][j] + by[a][i] -- two host tables,
// one fp32 addition -- and gives w(t, d) = max(0, 1 - |t - d|) of its value to bin d.  Both directions gather, so no sum depends on the order in
// which workgroups run: no atomics, equal from run to run.
//
// Forward, radon_fwd_kernel: a workgroup owns 256 bins (one per lane), kRadonAC angles and one image; the lane carries the kRadonAC partial sums in
// registers while the image passes through LDS band by band, so the image is read once per angle chunk, not once per angle.  The angles are split by
// the axis they walk: with |cos| >= |sin| the "major" axis is the image row and the "minor" axis the column, else the other way round; a chunk holds
// angles of one kind (RadonOp::order).  Along the minor axis t moves by the slope (cos or sin, at least 0.707 in magnitude) per pixel, so the pixels
// of one major line that reach bin d lie in an open interval of 2 / |slope| <= 2.83 minor pixels around u = (d - tmaj) / slope + (N - 1) / 2 (column
// kind: d less the detector's origin (n_det - 1) / 2, which its minor table by carries): the integers of (u - 1.415, u + 1.415) are among
// floor(u) - 1 .. floor(u) + 2, and they still are when the fp32 estimate of u is off by 0.4.  Its error
// is about 2^-22 (|d - tmaj| + side / 2) / |slope|, under 0.3 for sides up to kRadonMaxSide.  The lane evaluates w at those four candidates with the
// table values themselves, so a candidate outside the interval gets exactly 0 and which four were tried does not show in the sum.
// LDS (dynamic, kRadonLds floats): the major table of the band's lines, [MB][kRadonAC] (every lane reads the same address), the minor table of the
// chunk's angles, [kRadonAC][nb + 1], then the band, [MB][(nb + 1) | 1] (odd stride: the transposed staging of the column kind writes without bank
// conflicts).  The extra entry of both is a sentinel that gives weight 0 and value 0: a candidate outside the tile is sent there.  Images wider than kRadonNB minor pixels pass as several minor tiles; a candidate outside
// the tile at hand is skipped there and met in its own tile.
//
// Adjoint, radon_adj_kernel: a lane owns one pixel of a 16 x 16 tile and walks the angles: floor(t), two weights, two sinogram reads.  Out-of-range
// bins are dropped by a zero weight on a clamped address, so the loads do not sit under run-time conditions.
//
// The epilogue is a template parameter (RadonEpi, lmc_launch.h).
#pragma once
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kRadonAC = 8;                    // angles of one chunk = partial sums a lane carries
constexpr int kRadonBins = 256;                // bins of one workgroup = its lanes
constexpr int kRadonNB = 1024;                 // minor pixels of one staged tile at most
constexpr int kRadonLds = 15872;               // floats of the tables and the band: 62 KiB, two workgroups per CU
constexpr int kRadonRed = 8;                   // floats in front of them: the four float64 wave sums of the energy epilogues
constexpr int kRadonTile = 16;                 // adjoint: pixel tile side
constexpr float kRadonFar = 3.0e38f;           // the sentinel of the minor table: finite, and 1 - |kRadonFar + tmaj - d| < 0 for every table value
static_assert(kRadonLds - kRadonAC * (kRadonNB + 1) >= ((kRadonNB + 1) | 1) + kRadonAC, "a band holds at least one major line");
static_assert(kRadonAC % 4 == 0 && kRadonRed % 4 == 0, "the major table is read as float4");

struct RadonArgs {
  const float* x;       // forward: [C][H][W] image; adjoint: [C][na][nd] sinogram
  float* out;           // forward: [C][na][nd]; adjoint: [C][H][W]
  const float* xin;     // kRadonOverwrite: [C][H][W]
  const float* y;       // [na][nd] or [2][na][nd], shared by the images
  const float* tab;     // RadonOp::tab_dev
  double* part;         // energies: [C][gridDim.x]
  int H, W, na, nd, n_row;
  float a, coef;
};

// the weight of the definition, fp32 as written: both directions call this
__device__ __forceinline__ float radon_w(float t, float d) { return fmaxf(0.f, 1.f - fabsf(t - d)); }

template <int EPI>
__global__ __launch_bounds__(kRadonBins) void radon_fwd_kernel(RadonArgs P) {
  // all LDS is dynamic and every carve a multiple of 16 bytes: a static array in front would shift the base the float4 reads below rely on
  extern __shared__ __attribute__((aligned(16))) float radon_lds_base[];
  constexpr bool kEnergy = EPI == kRadonEnL2 || EPI == kRadonEnPois || EPI == kRadonEnWl2 || EPI == kRadonEnHub;
  double* red = reinterpret_cast<double*>(radon_lds_base);      // [4], kRadonRed floats
  float* radon_lds = radon_lds_base + kRadonRed;
  const int tid = threadIdx.x;
  const int H = P.H, W = P.W, na = P.na, nd = P.nd;
  const int bts = (nd + kRadonBins - 1) / kRadonBins;
  const int chunk = blockIdx.x / bts, bt = blockIdx.x - chunk * bts;
  const int rc = (P.n_row + kRadonAC - 1) / kRadonAC;
  const bool row = chunk < rc;                                  // the chunk's angles walk image rows
  const int first = row ? chunk * kRadonAC : P.n_row + (chunk - rc) * kRadonAC;
  const int cnt = min(kRadonAC, (row ? P.n_row : na) - first);
  const int Nmaj = row ? H : W, Nmin = row ? W : H;
  const float* __restrict__ tmajT = P.tab + (row ? (size_t)na * W : (size_t)0);      // by[a][i] / ax[a][j]
  const float* __restrict__ tminT = P.tab + (row ? (size_t)0 : (size_t)na * W);      // ax[a][j] / by[a][i]
  const float* __restrict__ inv = P.tab + (size_t)na * ((size_t)W + H);
  const int* __restrict__ order = reinterpret_cast<const int*>(inv + na);
  // (a short chunk repeats its last angle: computed, never stored)
  float invk[kRadonAC], acc[kRadonAC];
#pragma unroll
  for (int k = 0; k < kRadonAC; ++k) {
    invk[k] = inv[order[first + min(k, cnt - 1)]];
    acc[k] = 0.f;
  }
  const int d = bt * kRadonBins + tid;
  const float df = (float)d, cmin = 0.5f * (float)(Nmin - 1), umax = (float)Nmin + 4.f;
  // the minor table of the column kind is by, which carries the detector's origin (n_det - 1) / 2: taken off the bin before the estimate (exact)
  const float du = row ? df : df - 0.5f * (float)(nd - 1);
  const float* __restrict__ xi = P.x + (size_t)blockIdx.y * H * W;
  // Both LDS tables carry one sentinel behind the nb entries of a tile: a minor-table value so large that w is exactly 0, and an image value 0.  A
  // candidate outside the tile is sent there by one unsigned minimum, so the inner loop holds no comparison and no select.
  const int nbm = min(Nmin, kRadonNB), T = nbm + 1, S = T | 1;
  const int MB = min(Nmaj, (kRadonLds - kRadonAC * T) / (S + kRadonAC));
  float* tjS = radon_lds;                      // [MB][kRadonAC]: the major table of the band's lines
  float* tmS = tjS + MB * kRadonAC;            // [kRadonAC][T]: the minor table of the tile
  float* xs = tmS + kRadonAC * T;              // [MB][S]: the band
  for (int n0 = 0; n0 < Nmin; n0 += nbm) {
    const int nb = min(nbm, Nmin - n0), nb1 = nb + 1;
    __syncthreads();                                            // the readers of the previous minor table are done
    for (int e = tid; e < kRadonAC * nb1; e += kRadonBins) {
      const int k = e / nb1, c = e - k * nb1;
      tmS[k * T + c] = c < nb ? tminT[(size_t)order[first + min(k, cnt - 1)] * Nmin + n0 + c] : kRadonFar;
    }
    for (int m0 = 0; m0 < Nmaj; m0 += MB) {
      const int mb = min(MB, Nmaj - m0);
      __syncthreads();                                          // the readers of the previous band are done
      for (int e = tid; e < mb * kRadonAC; e += kRadonBins) {
        const int r = e / kRadonAC, k = e - r * kRadonAC;
        tjS[e] = tmajT[(size_t)order[first + min(k, cnt - 1)] * Nmaj + m0 + r];
      }
      if (row) {
        for (int e = tid; e < mb * nb1; e += kRadonBins) {
          const int r = e / nb1, c = e - r * nb1;
          xs[r * S + c] = c < nb ? xi[(size_t)(m0 + r) * W + n0 + c] : 0.f;
        }
      } else {                                                  // major = image column: read along the image row, write transposed
        for (int e = tid; e < mb * nb1; e += kRadonBins) {
          const int c = e / mb, r = e - c * mb;
          xs[r * S + c] = c < nb ? xi[(size_t)(n0 + c) * W + m0 + r] : 0.f;
        }
      }
      __syncthreads();
      for (int r = 0; r < mb; ++r) {
        const float* __restrict__ xr = xs + r * S;
        float tmk[kRadonAC];                                    // the same address in every lane: two broadcast reads
#pragma unroll
        for (int k4 = 0; k4 < kRadonAC; k4 += 4) {
          const float4 v = *reinterpret_cast<const float4*>(tjS + r * kRadonAC + k4);
          tmk[k4] = v.x; tmk[k4 + 1] = v.y; tmk[k4 + 2] = v.z; tmk[k4 + 3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < kRadonAC; ++k) {
          const float tm = tmk[k];
          const float u = fminf(fmaxf(fmaf(du - tm, invk[k], cmin), -4.f), umax);
          const int j0 = (int)floorf(u) - 1 - n0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int jc = (int)min((unsigned)(j0 + q), (unsigned)nb);      // (a negative index wraps to a large one: the sentinel too)
            const float t = tmS[k * T + jc] + tm;
            acc[k] = fmaf(radon_w(t, df), xr[jc], acc[k]);
          }
        }
      }
    }
  }
  const size_t pl = (size_t)na * nd;
  double fa = 0.0;
  if (d < nd) {
#pragma unroll
    for (int k = 0; k < kRadonAC; ++k) {
      if (k < cnt) {
        const size_t p = (size_t)order[first + k] * nd + d, o = (size_t)blockIdx.y * pl + p;
        const float u = acc[k];
        if constexpr (EPI == kRadonRaw) P.out[o] = u;
        if constexpr (EPI == kRadonRhoL2) P.out[o] = u - P.y[p];
        if constexpr (EPI == kRadonRhoPois) P.out[o] = pois_rho(u, P.y[p], P.y[pl + p]);
        if constexpr (EPI == kRadonRhoWl2) P.out[o] = P.y[pl + p] * (u - P.y[p]);
        if constexpr (EPI == kRadonRhoHub) P.out[o] = hub_psi(u - P.y[p], P.y[pl + p]);
        if constexpr (EPI == kRadonEnL2) { const double e = (double)u - (double)P.y[p]; fa += 0.5 * e * e; }
        if constexpr (EPI == kRadonEnPois) fa += pois_phi(u, P.y[p], P.y[pl + p]);
        if constexpr (EPI == kRadonEnWl2) { const double e = (double)u - (double)P.y[p]; fa += 0.5 * (double)P.y[pl + p] * e * e; }
        if constexpr (EPI == kRadonEnHub) fa += hub_h(u - P.y[p], P.y[pl + p]);
      }
    }
  }
  if constexpr (kEnergy) {      // a fixed order: lanes by shuffles, then the four waves by thread 0
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) fa += __shfl_down(fa, off, kWave);
    if ((tid & (kWave - 1)) == 0) red[tid >> 6] = fa;
    __syncthreads();
    if (tid == 0) P.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

template <int EPI>
__global__ __launch_bounds__(kRadonTile* kRadonTile) void radon_adj_kernel(RadonArgs P) {
  const int H = P.H, W = P.W, na = P.na, nd = P.nd;
  const int tiles_x = (W + kRadonTile - 1) / kRadonTile;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int i = tyi * kRadonTile + (threadIdx.x >> 4), j = txi * kRadonTile + (threadIdx.x & (kRadonTile - 1));
  const bool in = i < H && j < W;
  const int ic = min(i, H - 1), jc = min(j, W - 1);
  const float* __restrict__ ax = P.tab + jc;
  const float* __restrict__ by = P.tab + (size_t)na * W + ic;
  const float* __restrict__ r = P.x + (size_t)blockIdx.y * na * nd;
  const float fmax_d = (float)nd + 1.f;
  float s = 0.f;
#pragma unroll 4
  for (int a = 0; a < na; ++a) {
    const float t = ax[(size_t)a * W] + by[(size_t)a * H];
    const float f = fminf(fmaxf(floorf(t), -2.f), fmax_d);      // (clamped: both bins are then outside the detector)
    const int d0 = (int)f;
    const bool in0 = (unsigned)d0 < (unsigned)nd, in1 = (unsigned)(d0 + 1) < (unsigned)nd;
    const float w0 = in0 ? radon_w(t, f) : 0.f, w1 = in1 ? radon_w(t, f + 1.f) : 0.f;
    const float* __restrict__ ra = r + (size_t)a * nd;
    s = fmaf(w0, ra[in0 ? d0 : 0], s);
    s = fmaf(w1, ra[in1 ? d0 + 1 : 0], s);
  }
  if (in) {
    const size_t o = (size_t)blockIdx.y * H * W + (size_t)i * W + j;
    if constexpr (EPI == kRadonRaw) P.out[o] = s;
    if constexpr (EPI == kRadonSub) P.out[o] = fmaf(-P.coef, s, P.out[o]);
    if constexpr (EPI == kRadonOverwrite) P.out[o] = fmaf(-P.coef, s, P.a * P.xin[o]);
  }
}

// f_out[c] += scale * sum_b part[c][b], b in order: one lane per image
__global__ __launch_bounds__(256) void radon_energy_finish_kernel(const double* __restrict__ part, int64_t n_img, int blocks, double scale,
                                                                  double* __restrict__ f_out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_img) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)c * blocks + b];
  f_out[c] += scale * s;
}

}  // namespace lmc
