// Second-order total generalised variation (LMC_PRIOR_TGV; include/lmc_atomi.h holds the definition):
//   g(x) = sigma * min_w ( sum |grad x - w|_2 + alpha0 * sum |E w|_F )
// and its prox by a fixed number of Chambolle-Pock primal-dual iterations on (u, w) and the duals (p, q).
//   tgv_prox_kernel<BOX>   one workgroup = one 64 x 64 patch (tile + halo) of ONE image.  A lane holds v, grad v, the displacement d = u - v, w and the
//                          duals p, q of its four pixels in registers (44 floats); the iteration runs on d, whose size is that of the prox parameter and
//                          not of the image, so float32 rounds that much finer (u' - v = (d + s div p) / (1 + s); grad ub = grad v + grad db).  What
//                          neighbours read lives in LDS: the extrapolated primal (db = ub - v, w1b, w2b), read at +1 by the dual
//                          step, and the projected duals (p1, p2, q11, q22, q12), read at -1 by the primal step -- eight planes of 66 x 64 floats, 132 KB
//                          of the 160 KB, one workgroup per CU.  One patch row is one wave, so every neighbour read is a row of consecutive words.
//                          Information moves one pixel per iteration (p reads ub at +1, u reads p at -1; likewise q and w), so a launch of K iterations
//                          has a halo of K.  Up to kTgvLaunchIters iterations per launch; more are chained launches that carry (d, db, w1, w1b, w2, w2b,
//                          p1, p2, q11, q22, q12) -- 11 planes -- through two ping-pong work buffers exactly: neighbouring tiles read each other's
//                          previous state.  Two barriers per iteration, no atomics: equal runs give equal bits.
// Recompute: a launch of 6 iterations owns a 52 x 52 tile of its 64 x 64 patch, (64 / 52)^2 = 1.51 pixel updates per pixel of the image.  Measured at
// 512^2 x 1024 images, 40 iterations (scripts/bench_tgv.py): 71.8, 67.2, 70.5, 76.9 ms with 5, 6, 8, 10 iterations per launch -- fewer launches move the
// 88 B per pixel of state less often, longer launches recompute more halo.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kTgvThreads = 1024;
constexpr int kTgvPH = 64, kTgvPW = 64;      // the patch: one wave = one patch row
constexpr int kTgvLdsPlanes = 8;
constexpr int kTgvStatePlanes = 11;
constexpr size_t kTgvLdsBytes = (size_t)kTgvLdsPlanes * (kTgvPH + 2) * kTgvPW * sizeof(float);
static_assert(kTgvLdsBytes <= 160 * 1024, "a patch fits the LDS of one workgroup");
static_assert(2 * kTgvLaunchIters < kTgvPH && 2 * kTgvLaunchIters < kTgvPW, "the halo of a launch leaves a tile");

struct TgvArgs {
  int H, W;
  int tiles_x, tiles_y, TH, TW, HL;
  int niter;                  // iterations of this launch
  float s, inv1s;             // the step of both sides, 1 / (1 + s)
  float lam1, lam1sq;         // radius of the first-order ball, t sigma, and its square
  float lam0, lam0sq;         // radius of the second-order ball, alpha0 t sigma, and its square
  float box_lo, box_hi;
  const float* x;             // v, the point the prox is taken at
  float* out;                 // u of the last launch; NULL: a non-final launch of a chain, the state alone
  float* w_out;               // [n][2][H][W], the auxiliary field of the last launch; NULL: not asked for
  const float* st_in;         // [n][11][H][W], the state of the previous launch; NULL: u = ub = v (d = db = 0), everything else zero
  float* st_out;              // NULL: do not store
};

// LDS: eight planes, each PH rows of 64 floats between two pad rows, so that the +-1 neighbour reads of patch-border pixels stay inside the allocation
// (their values never reach the tile: the halo covers the launch).  Pixels outside the image hold zero duals in LDS -- div and div2 then see p = q = 0
// above the first row and left of the first column -- and the has-down / has-right flags cut every forward difference at the last row / column.
template <bool BOX>
__global__ __launch_bounds__(kTgvThreads) void tgv_prox_kernel(const TgvArgs P) {
  constexpr int PH = kTgvPH, PW = kTgvPW;
  constexpr int NP = PH * PW / kTgvThreads;
  constexpr int npix = PH * PW, arr = (PH + 2) * PW;
  static_assert(NP * kTgvThreads == npix, "every lane owns NP pixels of the patch");
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int tiles = P.tiles_x * P.tiles_y;
  const int n = blockIdx.x / tiles;
  const int tile = blockIdx.x - n * tiles;
  const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
  const int H = P.H, W = P.W, HL = P.HL;
  const int row0 = ty * P.TH - HL, col0 = tx * P.TW - HL;     // image coordinates of patch pixel (0, 0)
  const size_t img = (size_t)H * W;
  float* const UB = lds + PW;
  float* const W1B = UB + arr;
  float* const W2B = W1B + arr;
  float* const P1 = W2B + arr;
  float* const P2 = P1 + arr;
  float* const Q11 = P2 + arr;
  float* const Q22 = Q11 + arr;
  float* const Q12 = Q22 + arr;

  // d = u - v: the iteration runs on the displacement, whose magnitude is that of lam1 and not of the image, so float32 rounding is that much smaller;
  // grad v enters once, as (gvx, gvy), and v again in the box and in the result u = v + d
  float v[NP], gvx[NP], gvy[NP], d[NP], w1[NP], w2[NP], p1[NP], p2[NP], q11[NP], q22[NP], q12[NP];
  float db0[NP];      // the extrapolated displacement a resumed launch starts from (LDS holds v first)
  int flags[NP];      // bit0 in image, bit1 has-down, bit2 has-right
  unsigned gidx[NP];      // pixel index inside the image (H W <= 2^30)
  const float* __restrict__ st = P.st_in ? P.st_in + (size_t)n * kTgvStatePlanes * img : nullptr;
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kTgvThreads;
    const int r = p / PW, c = p - r * PW;
    const int gr = row0 + r, gc = col0 + c;
    const bool in = (gr >= 0) & (gr < H) & (gc >= 0) & (gc < W);
    flags[m] = (in ? 1 : 0) | ((in && gr + 1 < H) ? 2 : 0) | ((in && gc + 1 < W) ? 4 : 0);
    gidx[m] = in ? (unsigned)gr * (unsigned)W + (unsigned)gc : 0u;
    v[m] = in ? P.x[(size_t)n * img + gidx[m]] : 0.f;
    float db = 0.f, w1b = 0.f, w2b = 0.f;
    d[m] = 0.f;
    w1[m] = w2[m] = p1[m] = p2[m] = q11[m] = q22[m] = q12[m] = 0.f;
    if (st && in) {      // resume: the state of the previous launch on the patch
      const float* s11 = st + gidx[m];
      d[m] = s11[0]; db = s11[img];
      w1[m] = s11[2 * img]; w1b = s11[3 * img];
      w2[m] = s11[4 * img]; w2b = s11[5 * img];
      p1[m] = s11[6 * img]; p2[m] = s11[7 * img];
      q11[m] = s11[8 * img]; q22[m] = s11[9 * img]; q12[m] = s11[10 * img];
    }
    UB[p] = v[m]; W1B[p] = w1b; W2B[p] = w2b;      // (v first, for its differences; then the extrapolated displacement)
    db0[m] = db;
  }
  for (int i = tid; i < 2 * PW * kTgvLdsPlanes; i += kTgvThreads) {      // the pad rows of every plane
    const int plane = i / (2 * PW), j = i - plane * 2 * PW;
    lds[plane * arr + (j < PW ? j : npix + j)] = 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kTgvThreads;
    gvx[m] = (flags[m] & 2) ? UB[p + PW] - v[m] : 0.f;
    gvy[m] = (flags[m] & 4) ? UB[p + 1] - v[m] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NP; ++m) UB[tid + m * kTgvThreads] = db0[m];
  __syncthreads();

  const float s = P.s, inv1s = P.inv1s;
  const float lam1 = P.lam1, lam1sq = P.lam1sq, lam0 = P.lam0, lam0sq = P.lam0sq;
  for (int k = 0; k < P.niter; ++k) {
    // dual: p <- P_lam1(p + s (grad ub - wb)),  q <- P_lam0(q + s E wb)
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      const int p = tid + m * kTgvThreads;
      const bool in = flags[m] & 1, dn = flags[m] & 2, rt = flags[m] & 4;
      const float ub = UB[p], a1 = W1B[p], a2 = W2B[p];      // (ub: the extrapolated displacement)
      const float gx = gvx[m] + (dn ? UB[p + PW] - ub : 0.f);
      const float gy = gvy[m] + (rt ? UB[p + 1] - ub : 0.f);
      const float z1 = fmaf(s, gx - a1, p1[m]);
      const float z2 = fmaf(s, gy - a2, p2[m]);
      const float n2 = fmaf(z1, z1, z2 * z2);
      const float sc1 = n2 > lam1sq ? lam1 * rsqrtf(n2) : 1.f;
      p1[m] = z1 * sc1;
      p2[m] = z2 * sc1;
      const float e11 = dn ? W1B[p + PW] - a1 : 0.f;
      const float ea = rt ? W1B[p + 1] - a1 : 0.f;
      const float eb = dn ? W2B[p + PW] - a2 : 0.f;
      const float e22 = rt ? W2B[p + 1] - a2 : 0.f;
      const float e12 = 0.5f * (ea + eb);
      const float y11 = fmaf(s, e11, q11[m]);
      const float y22 = fmaf(s, e22, q22[m]);
      const float y12 = fmaf(s, e12, q12[m]);
      const float m2 = fmaf(y11, y11, fmaf(y22, y22, 2.f * (y12 * y12)));
      const float sc0 = m2 > lam0sq ? lam0 * rsqrtf(m2) : 1.f;
      q11[m] = y11 * sc0;
      q22[m] = y22 * sc0;
      q12[m] = y12 * sc0;
      P1[p] = in ? p1[m] : 0.f;
      P2[p] = in ? p2[m] : 0.f;
      Q11[p] = in ? q11[m] : 0.f;
      Q22[p] = in ? q22[m] : 0.f;
      Q12[p] = in ? q12[m] : 0.f;
    }
    __syncthreads();
    // primal: u' = clip((u + s div p + s v) / (1 + s)) as d' = clip_{[lo - v, hi - v]}((d + s div p) / (1 + s)),  w' = w + s (p + div2 q);
    // db = 2 d' - d,  wb = 2 w' - w
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      const int p = tid + m * kTgvThreads;
      const bool dn = flags[m] & 2, rt = flags[m] & 4;
      const float dp = ((dn ? p1[m] : 0.f) - P1[p - PW]) + ((rt ? p2[m] : 0.f) - P2[p - 1]);
      float dnew = fmaf(s, dp, d[m]) * inv1s;      // u' - v = (u - v + s div p) / (1 + s)
      if constexpr (BOX) dnew = __builtin_amdgcn_fmed3f(dnew, P.box_lo - v[m], P.box_hi - v[m]);
      UB[p] = fmaf(2.f, dnew, -d[m]);
      d[m] = dnew;
      const float q12u = Q12[p - PW], q12l = Q12[p - 1];
      const float d1 = ((dn ? q11[m] : 0.f) - Q11[p - PW]) + ((rt ? q12[m] : 0.f) - q12l);
      const float d2 = ((dn ? q12[m] : 0.f) - q12u) + ((rt ? q22[m] : 0.f) - Q22[p - 1]);
      const float w1n = fmaf(s, p1[m] + d1, w1[m]);
      const float w2n = fmaf(s, p2[m] + d2, w2[m]);
      W1B[p] = fmaf(2.f, w1n, -w1[m]);
      W2B[p] = fmaf(2.f, w2n, -w2[m]);
      w1[m] = w1n;
      w2[m] = w2n;
    }
    __syncthreads();
  }

  // the tile: the patch without its halo, inside the image
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kTgvThreads;
    const int r = p / PW, c = p - r * PW;
    if (!(flags[m] & 1) || r < HL || r >= HL + P.TH || c < HL || c >= HL + P.TW) continue;
    if (P.st_out) {
      float* __restrict__ s11 = P.st_out + (size_t)n * kTgvStatePlanes * img + gidx[m];
      s11[0] = d[m]; s11[img] = UB[p];
      s11[2 * img] = w1[m]; s11[3 * img] = W1B[p];
      s11[4 * img] = w2[m]; s11[5 * img] = W2B[p];
      s11[6 * img] = p1[m]; s11[7 * img] = p2[m];
      s11[8 * img] = q11[m]; s11[9 * img] = q22[m]; s11[10 * img] = q12[m];
    }
    if (P.out) {
      float un = v[m] + d[m];
      if constexpr (BOX) un = __builtin_amdgcn_fmed3f(un, P.box_lo, P.box_hi);      // (d is inside [lo - v, hi - v]; the sum rounds once more)
      P.out[(size_t)n * img + gidx[m]] = un;
    }
    if (P.w_out) {
      float* __restrict__ wo = P.w_out + (size_t)n * 2 * img + gidx[m];
      wo[0] = w1[m]; wo[img] = w2[m];
    }
  }
}

// ---- host side --------------------------------------------------------------------------------

bool tgv_plan(int niter, TgvPlan& out) {
  if (niter < 1 || niter > kMaxTgvIters) return false;
  out.PH = kTgvPH; out.PW = kTgvPW;
  out.n_launches = (niter + kTgvLaunchIters - 1) / kTgvLaunchIters;
  out.iters = (niter + out.n_launches - 1) / out.n_launches;
  out.HL = out.iters;      // every launch starts from a complete state: a halo of K covers K iterations
  out.TH = out.PH - 2 * out.HL; out.TW = out.PW - 2 * out.HL;
  out.lds_bytes = kTgvLdsBytes;
  return true;
}

size_t tgv_state_floats(int64_t n_img, int H, int W, int niter) {
  TgvPlan pl;
  if (!tgv_plan(niter, pl) || pl.n_launches == 1) return 0;
  return (size_t)n_img * kTgvStatePlanes * H * W;
}

template <bool BOX>
static hipError_t tgv_launch_one(const TgvArgs& a, unsigned nblk, hipStream_t st) {
  static thread_local bool configured = false;
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tgv_prox_kernel<BOX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTgvLdsBytes);
    if (e != hipSuccess) return e;
    configured = true;
  }
  hipLaunchKernelGGL((tgv_prox_kernel<BOX>), dim3(nblk), dim3(kTgvThreads), kTgvLdsBytes, st, a);
  return hipGetLastError();
}

hipError_t launch_tgv_prox(const float* x, float* out, float* w_out, int64_t n_img, int H, int W, float lam1, float alpha0, float step, int niter, int box,
                           float box_lo, float box_hi, float* state0, float* state1, hipStream_t st) {
  TgvPlan pl;
  if (!x || !out || x == out || n_img < 1 || H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30) || !(lam1 > 0.f) || !(alpha0 > 0.f) || !(step > 0.f) ||
      !tgv_plan(niter, pl))
    return hipErrorInvalidValue;
  if (pl.n_launches > 1 && (!state0 || !state1)) return hipErrorInvalidValue;
  TgvArgs a{};
  a.H = H; a.W = W; a.TH = pl.TH; a.TW = pl.TW; a.HL = pl.HL;
  a.tiles_x = (W + pl.TW - 1) / pl.TW; a.tiles_y = (H + pl.TH - 1) / pl.TH;
  const int64_t nblk = (int64_t)a.tiles_x * a.tiles_y * n_img;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  a.s = step; a.inv1s = 1.f / (1.f + step);
  a.lam1 = lam1; a.lam1sq = lam1 * lam1;
  a.lam0 = alpha0 * lam1; a.lam0sq = a.lam0 * a.lam0;
  a.box_lo = box_lo; a.box_hi = box_hi;
  a.x = x;
  float* state[2] = {state0, state1};
  for (int l = 0; l < pl.n_launches; ++l) {
    const int k0 = l * pl.iters;
    const bool last = l == pl.n_launches - 1;
    a.niter = niter - k0 < pl.iters ? niter - k0 : pl.iters;
    a.st_in = l > 0 ? state[(l - 1) & 1] : nullptr;
    a.st_out = last ? nullptr : state[l & 1];
    a.out = last ? out : nullptr;
    a.w_out = last ? w_out : nullptr;
    const hipError_t e = box ? tgv_launch_one<true>(a, (unsigned)nblk, st) : tgv_launch_one<false>(a, (unsigned)nblk, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace lmc
