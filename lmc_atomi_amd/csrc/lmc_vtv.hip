// Vectorial total variation (LMC_PRIOR_VTV; include/lmc_atomi.h holds the definition): g(x) = sigma * sum_pixels sqrt(sum_ch (d_r x_ch)^2 + (d_c x_ch)^2)
// on a multi-channel image x[ch][H][W], its prox by fast-gradient-projection dual iterations and its value.
//   vtv_prox_kernel<NCH, BOX>   one workgroup = one patch (tile + halo) of ONE multi-channel image.  A lane owns all NCH channels of its NP pixels, so the
//                               one projection weight of a pixel, w = max(1, sqrt(sum_ch r_ch^2 + s_ch^2)), is lane-local: the channels couple in that line
//                               and nowhere else.  x and the projected dual (p, q) of the lane's pixels stay in registers; the extrapolated dual (rr, ss)
//                               and the primal iterate live in LDS per channel, where the +-1 neighbour reads find them (12 B per pixel and channel).  Up to kVtvLaunchIters
//                               dual iterations per launch; more are chained launches that carry (rr, ss, p, q) per channel through HBM exactly, as the
//                               tile kernel's tv_in / tv_out do.
//   vtv_value_kernel            partial sums of sqrt(sum_ch ...) in float64, one slot per workgroup; vtv_value_sum_kernel adds the slots of an image in
//                               slot order.  No atomics anywhere: equal runs give equal bits.
// Layout: channel-major, image (ch, n) at x + ch * channel_stride + n * H * W.
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kVtvThreads = 1024;
constexpr int kVtvPW = 64;               // patch columns (one wave = one patch row)
constexpr int kVtvLaunchIters = 10;      // dual iterations one launch holds (its halo)
constexpr int kVtvValueThreads = 256;

// patch rows by channel count: three arrays of (PH + 2) x 64 floats per channel within one workgroup's 160 KB of LDS
constexpr int vtv_patch_rows(int nch) { return nch == 4 ? 48 : 64; }
constexpr size_t vtv_lds_bytes(int nch) { return (size_t)3 * nch * (vtv_patch_rows(nch) + 2) * kVtvPW * sizeof(float); }
static_assert(vtv_lds_bytes(3) <= 160 * 1024 && vtv_lds_bytes(4) <= 160 * 1024, "a patch fits the LDS of one workgroup");

struct VtvArgs {
  int H, W;
  int tiles_x, tiles_y, TH, TW, HL;
  int niter;                  // dual iterations of this launch
  float gamma, c;             // t * sigma; dual step = step / gamma
  float betas[kVtvLaunchIters];
  float box_lo, box_hi;
  long long cs;               // channel stride of x and out, floats
  const float* x;
  float* out;                 // NULL: a non-final launch of a chain, the state alone
  const float* st_in;         // [n_img][NCH][4][H][W] = (rr, ss, p, q) of the previous launch; NULL: the zero dual
  float* st_out;              // NULL: do not store
};

// LDS per channel: S (primal iterate), A (dual, row component), B (dual, column component), each PH rows of 64 floats between two pad rows, so that
// the +-1 neighbour reads of patch-border pixels stay inside the allocation (their values never reach the tile: information moves one pixel per dual
// iteration and the halo covers the launch).  Pixels outside the image hold x = 0 (BOX: its clamp) and a zero dual; the has-down / has-right flags cut
// every difference with them.
template <int NCH, bool BOX>
__global__ __launch_bounds__(kVtvThreads) void vtv_prox_kernel(const VtvArgs P) {
  constexpr int PH = vtv_patch_rows(NCH), PW = kVtvPW;
  constexpr int NP = PH * PW / kVtvThreads;
  constexpr int npix = PH * PW, arr = (PH + 2) * PW;
  static_assert(NP * kVtvThreads == npix, "every lane owns NP pixels of the patch");
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int tiles = P.tiles_x * P.tiles_y;
  const int n = blockIdx.x / tiles;
  const int tile = blockIdx.x - n * tiles;
  const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
  const int H = P.H, W = P.W, HL = P.HL;
  const int row0 = ty * P.TH - HL, col0 = tx * P.TW - HL;     // image coordinates of patch pixel (0, 0)
  const size_t img = (size_t)H * W;
  float* const S0 = lds + PW;
  auto Sc = [&](int ch) { return S0 + (3 * ch) * arr; };
  auto Ac = [&](int ch) { return S0 + (3 * ch + 1) * arr; };
  auto Bc = [&](int ch) { return S0 + (3 * ch + 2) * arr; };

  float xv[NP][NCH], pv[NP][NCH], qv[NP][NCH];      // (rr, ss) of the lane's pixels: in LDS alone
  int flags[NP];      // bit0 in image, bit1 has-down, bit2 has-right
  unsigned gidx[NP];      // pixel index inside the image (H W <= 2^30)
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kVtvThreads;
    const int r = p / PW, c = p - r * PW;
    const int gr = row0 + r, gc = col0 + c;
    const bool in = (gr >= 0) & (gr < H) & (gc >= 0) & (gc < W);
    flags[m] = (in ? 1 : 0) | ((in && gr + 1 < H) ? 2 : 0) | ((in && gc + 1 < W) ? 4 : 0);
    gidx[m] = in ? (unsigned)gr * (unsigned)W + (unsigned)gc : 0u;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      xv[m][ch] = in ? P.x[(size_t)ch * P.cs + (size_t)n * img + gidx[m]] : 0.f;
      pv[m][ch] = qv[m][ch] = 0.f;
      Ac(ch)[p] = 0.f; Bc(ch)[p] = 0.f;
    }
  }
  for (int i = tid; i < PW; i += kVtvThreads) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      Ac(ch)[-PW + i] = 0.f; Bc(ch)[-PW + i] = 0.f; Ac(ch)[npix + i] = 0.f; Bc(ch)[npix + i] = 0.f;
      Sc(ch)[-PW + i] = 0.f; Sc(ch)[npix + i] = 0.f;
    }
  }
  __syncthreads();
  if (P.st_in) {      // resume: the dual state of the previous launch on the patch, zero outside the image
    const float* __restrict__ st = P.st_in + (size_t)n * NCH * 4 * img;
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      if (flags[m] & 1) {
        const int p = tid + m * kVtvThreads;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const float* s4 = st + (size_t)ch * 4 * img + gidx[m];
          Ac(ch)[p] = s4[0]; Bc(ch)[p] = s4[img]; pv[m][ch] = s4[2 * img]; qv[m][ch] = s4[3 * img];
        }
      }
    }
    __syncthreads();
  }

  const float gam = P.gamma, cstep = P.c;
  for (int k = 0; k <= P.niter; ++k) {
    if (k == P.niter && !P.out) break;      // a non-final launch returns no primal iterate
    // sol = clip(x - gamma div(rr, ss))
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      const int p = tid + m * kVtvThreads;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float dv = (Ac(ch)[p] - Ac(ch)[p - PW]) + (Bc(ch)[p] - Bc(ch)[p - 1]);
        float sol = fmaf(-gam, dv, xv[m][ch]);
        if constexpr (BOX) sol = __builtin_amdgcn_fmed3f(sol, P.box_lo, P.box_hi);
        Sc(ch)[p] = sol;
      }
    }
    __syncthreads();
    if (k == P.niter) break;
    const float beta = P.betas[k];
    // dual ascent step, ONE projection weight per pixel over all channels, momentum
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      const int p = tid + m * kVtvThreads;
      float r[NCH], s[NCH];
      float n2 = 0.f;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float sol = Sc(ch)[p];
        const float dx = (flags[m] & 2) ? Sc(ch)[p + PW] - sol : 0.f;
        const float dy = (flags[m] & 4) ? Sc(ch)[p + 1] - sol : 0.f;
        r[ch] = fmaf(-cstep, dx, Ac(ch)[p]);
        s[ch] = fmaf(-cstep, dy, Bc(ch)[p]);
        n2 = fmaf(r[ch], r[ch], fmaf(s[ch], s[ch], n2));
      }
      const float inv = rsqrtf(fmaxf(n2, 1.f));
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float pn = r[ch] * inv, qn = s[ch] * inv;
        Ac(ch)[p] = fmaf(beta, pn - pv[m][ch], pn);
        Bc(ch)[p] = fmaf(beta, qn - qv[m][ch], qn);
        pv[m][ch] = pn;
        qv[m][ch] = qn;
      }
    }
    __syncthreads();
  }

  // the tile: the patch without its halo, inside the image
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kVtvThreads;
    const int r = p / PW, c = p - r * PW;
    if (!(flags[m] & 1) || r < HL || r >= HL + P.TH || c < HL || c >= HL + P.TW) continue;
    if (P.st_out) {
      float* __restrict__ st = P.st_out + (size_t)n * NCH * 4 * img;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        float* s4 = st + (size_t)ch * 4 * img + gidx[m];
        s4[0] = Ac(ch)[p]; s4[img] = Bc(ch)[p]; s4[2 * img] = pv[m][ch]; s4[3 * img] = qv[m][ch];
      }
    }
    if (P.out) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) P.out[(size_t)ch * P.cs + (size_t)n * img + gidx[m]] = Sc(ch)[p];
    }
  }
}

// part[n * n_seg + seg] = the sum over the pixels [seg * chunk, (seg + 1) * chunk) of image n of sqrt(sum_ch (d_r x_ch)^2 + (d_c x_ch)^2): fp32 forward
// differences (zero in the last row / column) and squares, the root and the sum in float64
__global__ __launch_bounds__(kVtvValueThreads) void vtv_value_kernel(const float* __restrict__ x, int nch, long long cs, int H, int W, long long chunk,
                                                                     int n_seg, double* __restrict__ part) {
  __shared__ double scratch[kVtvValueThreads / kWave];
  const size_t n = blockIdx.x / n_seg;
  const int seg = blockIdx.x - (int)n * n_seg;
  const long long img = (long long)H * W;
  const long long k0 = seg * chunk, k1 = min(k0 + chunk, img);
  double acc = 0.0;
  for (long long k = k0 + threadIdx.x; k < k1; k += kVtvValueThreads) {
    const int i = (int)(k / W), j = (int)(k - (long long)i * W);
    float n2 = 0.f;
    for (int ch = 0; ch < nch; ++ch) {
      const float* xc = x + (size_t)ch * cs + n * img + k;
      const float v = xc[0];
      const float dr = i + 1 < H ? xc[W] - v : 0.f;
      const float dc = j + 1 < W ? xc[1] - v : 0.f;
      n2 = fmaf(dr, dr, fmaf(dc, dc, n2));
    }
    acc += sqrt((double)n2);
  }
  const double tot = block_sum(acc, scratch);
  if (threadIdx.x == 0) part[n * n_seg + seg] = tot;
}

__global__ __launch_bounds__(256) void vtv_value_sum_kernel(const double* __restrict__ part, long long n_img, int n_seg, double scale, double* __restrict__ val) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_img) return;
  double a = 0.0;
  for (int k = 0; k < n_seg; ++k) a += part[(size_t)i * n_seg + k];
  val[i] = scale * a;
}

// ---- host side --------------------------------------------------------------------------------

bool vtv_plan(int nch, int niter, VtvPlan& out) {
  if (nch < 1 || nch > kVtvMaxChannels || niter < 1 || niter > kMaxTvIters) return false;
  out.PH = vtv_patch_rows(nch); out.PW = kVtvPW;
  if (niter <= kVtvLaunchIters) {      // from the zero dual the first primal iterate is x itself: a halo of K covers K iterations
    out.n_launches = 1; out.iters = niter; out.HL = niter;
  } else {                             // a launch that resumes forms x - gamma div(state) first, which reaches one pixel up / left: K + 1
    out.n_launches = (niter + kVtvLaunchIters - 2) / (kVtvLaunchIters - 1);
    out.iters = (niter + out.n_launches - 1) / out.n_launches;
    out.HL = out.iters + 1;
  }
  out.TH = out.PH - 2 * out.HL; out.TW = out.PW - 2 * out.HL;
  out.lds_bytes = vtv_lds_bytes(nch);
  return true;
}

size_t vtv_state_floats(int64_t n_img, int nch, int H, int W, int niter) {
  VtvPlan pl;
  if (!vtv_plan(nch, niter, pl) || pl.n_launches == 1) return 0;
  return (size_t)n_img * nch * 4 * H * W;
}

template <int NCH, bool BOX>
static hipError_t vtv_launch_one(const VtvArgs& a, unsigned nblk, hipStream_t st) {
  static thread_local bool configured = false;
  constexpr size_t lds = vtv_lds_bytes(NCH);
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vtv_prox_kernel<NCH, BOX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    configured = true;
  }
  hipLaunchKernelGGL((vtv_prox_kernel<NCH, BOX>), dim3(nblk), dim3(kVtvThreads), lds, st, a);
  return hipGetLastError();
}

template <bool BOX>
static hipError_t vtv_launch_nch(int nch, const VtvArgs& a, unsigned nblk, hipStream_t st) {
  switch (nch) {
    case 1: return vtv_launch_one<1, BOX>(a, nblk, st);
    case 2: return vtv_launch_one<2, BOX>(a, nblk, st);
    case 3: return vtv_launch_one<3, BOX>(a, nblk, st);
    case 4: return vtv_launch_one<4, BOX>(a, nblk, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_vtv_prox(const float* x, float* out, int64_t n_img, int nch, int64_t cs, int H, int W, float gamma, float step, const float* betas, int niter,
                           int box, float box_lo, float box_hi, float* state0, float* state1, hipStream_t st) {
  VtvPlan pl;
  if (!x || !out || x == out || n_img < 1 || H < 1 || W < 1 || !betas || !(gamma > 0.f) || !(step > 0.f) || !vtv_plan(nch, niter, pl)) return hipErrorInvalidValue;
  if (nch > 1 && cs < n_img * (int64_t)H * W) return hipErrorInvalidValue;
  if (pl.n_launches > 1 && (!state0 || !state1)) return hipErrorInvalidValue;
  VtvArgs a{};
  a.H = H; a.W = W; a.TH = pl.TH; a.TW = pl.TW; a.HL = pl.HL;
  a.tiles_x = (W + pl.TW - 1) / pl.TW; a.tiles_y = (H + pl.TH - 1) / pl.TH;
  const int64_t nblk = (int64_t)a.tiles_x * a.tiles_y * n_img;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  a.gamma = gamma; a.c = step / gamma;
  a.box_lo = box_lo; a.box_hi = box_hi;
  a.cs = cs; a.x = x;
  float* state[2] = {state0, state1};
  for (int l = 0; l < pl.n_launches; ++l) {
    const int k0 = l * pl.iters, kn = niter - k0 < pl.iters ? niter - k0 : pl.iters;
    const bool last = l == pl.n_launches - 1;
    a.niter = kn;
    for (int i = 0; i < kn; ++i) a.betas[i] = betas[k0 + i];
    a.st_in = l > 0 ? state[(l - 1) & 1] : nullptr;
    a.st_out = last ? nullptr : state[l & 1];
    a.out = last ? out : nullptr;
    const hipError_t e = box ? vtv_launch_nch<true>(nch, a, (unsigned)nblk, st) : vtv_launch_nch<false>(nch, a, (unsigned)nblk, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// slots of one image: chunks of at least 16384 pixels, 256 at the most
int vtv_value_segments(int H, int W) {
  const int64_t img = (int64_t)H * W;
  const int64_t s = (img + 16383) / 16384;
  return (int)(s < 1 ? 1 : (s > 256 ? 256 : s));
}

size_t vtv_value_partials(int64_t n_img, int H, int W) { return (size_t)n_img * vtv_value_segments(H, W); }

hipError_t launch_vtv_value(const float* x, int64_t n_img, int nch, int64_t cs, int H, int W, double scale, double* part, double* val, hipStream_t st) {
  if (!x || !part || !val || n_img < 1 || H < 1 || W < 1 || nch < 1 || nch > kVtvMaxChannels) return hipErrorInvalidValue;
  const int n_seg = vtv_value_segments(H, W);
  const int64_t img = (int64_t)H * W, chunk = (img + n_seg - 1) / n_seg;
  const int64_t nblk = n_img * n_seg;
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vtv_value_kernel, dim3((unsigned)nblk), dim3(kVtvValueThreads), 0, st, x, nch, (long long)cs, H, W, (long long)chunk, n_seg, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vtv_value_sum_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, st, part, (long long)n_img, n_seg, scale, val);
  return hipGetLastError();
}

}  // namespace lmc
