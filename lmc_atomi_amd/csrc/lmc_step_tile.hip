// Fused MYULA update, LDS-tiled variant ("tile"): one workgroup = one (TH x TW) output tile of
// one chain.  out = a*x - t*grad f(x) + b*prox_g(x) + s*xi, everything between the HBM read of
// x (tile + halo) and the HBM write of x' stays on chip:
//   * blur residual R = Hx - y and its adjoint H^T R from LDS-staged stencils,
//   * K fast-gradient-projection iterations of the TV prox with the dual field in LDS/registers,
//   * Philox4x32-10 + Box-Muller noise in registers (one call per 4 vertically adjacent pixels).
// Reference update: algs.py:569 (MoreauYosidaUnadjustedLangevin).
#include "lmc_device.h"
#include "lmc_launch.h"

namespace lmc {

constexpr int kStepThreads = 1024;

// One inclusion per data term gives its two kernels, LMC_TILE_NAME(_kernel)<NP, TV, ANISO> (every prior) and LMC_TILE_NAME(_box_kernel)<NP, ANISO> (the
// box-constrained TV prior, either form): names and instruction streams as they were when each was a block of its own
#define LMC_TILE_TERM kTermL2
#define LMC_TILE_NAME(sfx) myula_step_tile##sfx
#include "lmc_step_tile_kernel.h"
#undef LMC_TILE_TERM
#undef LMC_TILE_NAME
#define LMC_TILE_TERM kTermPois
#define LMC_TILE_NAME(sfx) myula_step_tile_pois##sfx
#include "lmc_step_tile_kernel.h"
#undef LMC_TILE_TERM
#undef LMC_TILE_NAME
#define LMC_TILE_TERM kTermWl2
#define LMC_TILE_NAME(sfx) myula_step_tile_wl2##sfx
#include "lmc_step_tile_kernel.h"
#undef LMC_TILE_TERM
#undef LMC_TILE_NAME
#define LMC_TILE_TERM kTermHub
#define LMC_TILE_NAME(sfx) myula_step_tile_hub##sfx
#include "lmc_step_tile_kernel.h"
#undef LMC_TILE_TERM
#undef LMC_TILE_NAME

// ---- host-side launcher --------------------------------------------------------------------

struct TilePlan {
  int TH, TW, HL, PH, PW, NP;
  size_t lds_bytes;
};

static bool plan_tiles(int H, int W, int halo, bool tv, size_t lds_limit, TilePlan& out) {
  const int n_arr = tv ? 4 : 2;
  // candidate output tiles, largest first; TW*TH/4 <= 1024 threads, TH % 4 == 0
  static const int cand[][2] = {{64, 64}, {48, 64}, {32, 64}, {32, 32}, {16, 32}, {16, 16}, {8, 16}, {4, 16}};
  for (auto& c : cand) {
    const int TH = c[0], TW = c[1];
    const int PH = TH + 2 * halo, PW = TW + 2 * halo;
    const size_t bytes = (size_t)n_arr * (PH + 2) * PW * sizeof(float) + 64;
    const int NP = (PH * PW + kStepThreads - 1) / kStepThreads;
    if (bytes <= lds_limit && NP <= 8) {
      out = {TH, TW, halo, PH, PW, NP, bytes};
      return true;
    }
  }
  return false;
}

template <auto k>
static hipError_t launch_kernel(const StepArgs& a, size_t lds, hipStream_t st) {
  static thread_local size_t configured = 0;
  if (lds > configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    configured = lds;
  }
  const int nblk = a.tiles_x * a.tiles_y * a.C;
  hipLaunchKernelGGL(k, dim3(nblk), dim3(kStepThreads), lds, st, a);
  return hipGetLastError();
}

// the kernel of a term: the box-constrained one where the prior is TV and the box is on
template <int TERM, int NP, bool TV, bool ANISO, bool BOX>
static constexpr auto tile_kernel() {
#define LMC_TILE_PICK(name) if constexpr (BOX) return name##_box_kernel<NP, ANISO>; else return name##_kernel<NP, TV, ANISO>;
  if constexpr (TERM == kTermPois) { LMC_TILE_PICK(myula_step_tile_pois) }
  else if constexpr (TERM == kTermWl2) { LMC_TILE_PICK(myula_step_tile_wl2) }
  else if constexpr (TERM == kTermHub) { LMC_TILE_PICK(myula_step_tile_hub) }
  else { LMC_TILE_PICK(myula_step_tile) }
#undef LMC_TILE_PICK
}

template <int TERM, int NP, bool TV, bool ANISO>
static hipError_t launch_term(const StepArgs& a, size_t lds, hipStream_t st) {
  if constexpr (TV) {
    if (a.box) return launch_kernel<tile_kernel<TERM, NP, TV, ANISO, true>()>(a, lds, st);
  }
  return launch_kernel<tile_kernel<TERM, NP, TV, ANISO, false>()>(a, lds, st);
}

template <int NP, bool TV, bool ANISO>
static hipError_t launch_np(const StepArgs& a, size_t lds, hipStream_t st) {
  switch (a.term) {
    case kTermPois: return launch_term<kTermPois, NP, TV, ANISO>(a, lds, st);
    case kTermWl2: return launch_term<kTermWl2, NP, TV, ANISO>(a, lds, st);
    case kTermHub: return launch_term<kTermHub, NP, TV, ANISO>(a, lds, st);
    default: return launch_term<kTermL2, NP, TV, ANISO>(a, lds, st);
  }
}

template <bool TV, bool ANISO = false>
static hipError_t launch_tv(const StepArgs& a, int NP, size_t lds, hipStream_t st) {
  switch (NP) {
    case 1: return launch_np<1, TV, ANISO>(a, lds, st);
    case 2: return launch_np<2, TV, ANISO>(a, lds, st);
    case 3: return launch_np<3, TV, ANISO>(a, lds, st);
    case 4: return launch_np<4, TV, ANISO>(a, lds, st);
    case 5: return launch_np<5, TV, ANISO>(a, lds, st);
    case 6: return launch_np<6, TV, ANISO>(a, lds, st);
    case 7: return launch_np<7, TV, ANISO>(a, lds, st);
    case 8: return launch_np<8, TV, ANISO>(a, lds, st);
  }
  return hipErrorInvalidValue;
}

// Fills the tile geometry of `a` (needs H, W, data/prior fields set) and launches.
// Returns hipErrorInvalidConfiguration if no tile fits (halo too large).
hipError_t launch_step_tile(StepArgs a, hipStream_t st) {
  const bool tv = a.prior_kind == LMC_PRIOR_TV_ISO;
  if (a.box && (!tv || !(a.box_lo < a.box_hi))) return hipErrorInvalidConfiguration;   // (separable priors take their box before the step: launch_box_prox)
  int halo = 0;
  if (a.data_kind == LMC_DATA_BLUR) halo = max(a.blur.kh, a.blur.kw) - 1;
  // Dual iterations spread one pixel per iteration in every direction: K iterations from the ZERO dual state leave sol^K valid on the tile when the
  // halo is K (the first primal iterate is x itself).  A chunk that RESUMES from a stored state first forms sol^0 = x - gamma div(state), which already
  // reaches one pixel up / left: it needs K + 1.  (Round 3: with a halo of K the final chunk's prox was wrong along the top row / left column of every
  // tile by an amount that decays ~6x per iteration of that chunk -- 1e-3 for a last chunk of one iteration (K = 17), 1e-9 for a full one.)
  if (tv) halo = max(halo, a.tv.niter + (a.tv_in ? 1 : 0));
  if (a.ncvx_kind != LMC_NCVX_NONE) halo = max(halo, 1);
  TilePlan tp;
  if (!plan_tiles(a.H, a.W, halo, tv, 160 * 1024, tp)) return hipErrorInvalidConfiguration;
  a.TH = tp.TH; a.TW = tp.TW; a.HL = tp.HL; a.PH = tp.PH; a.PW = tp.PW;
  a.tiles_x = (a.W + tp.TW - 1) / tp.TW;
  a.tiles_y = (a.H + tp.TH - 1) / tp.TH;
  if (tv && a.tv_aniso) return launch_tv<true, true>(a, tp.NP, tp.lds_bytes, st);
  return tv ? launch_tv<true>(a, tp.NP, tp.lds_bytes, st) : launch_tv<false>(a, tp.NP, tp.lds_bytes, st);
}


// TV prox with more dual iterations than one launch's halo allows: chunks of <= kTvChunk iterations chained exactly
// through the dual state (rr, ss, p, q) in HBM (two ping-pong buffers of [C][4][H][W] floats each).  Non-final chunks
// only advance the state; the final chunk also does the blur gradient, the combine and the store.
constexpr int kTvChunk = 8;

bool tile_needs_chunks(const StepArgs& a) {
  return a.prior_kind == LMC_PRIOR_TV_ISO && a.tv.niter > 12;
}

hipError_t launch_step_tile_chunked(const StepArgs& a, float* state0, float* state1, hipStream_t st) {
  const int K = a.tv.niter;
  const int n_chunks = (K + kTvChunk - 1) / kTvChunk;
  float* state[2] = {state0, state1};
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int k0 = ch * kTvChunk, kn = (K - k0 < kTvChunk) ? K - k0 : kTvChunk;
    const bool last = ch == n_chunks - 1;
    StepArgs b = a;
    b.tv.niter = kn;
    for (int i = 0; i < kn; ++i) b.tv.betas[i] = a.tv.betas[k0 + i];
    b.tv_in = ch > 0 ? state[(ch - 1) & 1] : nullptr;
    b.tv_out = last ? nullptr : state[ch & 1];
    b.tv_state_only = last ? 0 : 1;
    if (!last) { b.data_kind = LMC_DATA_NONE; b.term = kTermL2; b.ncvx_kind = LMC_NCVX_NONE; b.extra = nullptr; }
    hipError_t e = launch_step_tile(b, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// per-image sum of squared differences ||a_i - b_i||^2 (ME-TV envelope value), one atomic per block
__global__ __launch_bounds__(256) void sqdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t img,
                                                     double* __restrict__ out) {
  __shared__ double scratch[4];
  const size_t c = blockIdx.x;      // images on gridDim.x (no 65535 limit)
  double acc = 0.0;
  for (size_t k = (size_t)blockIdx.y * blockDim.x + threadIdx.x; k < img; k += (size_t)gridDim.y * blockDim.x) {
    const double d = (double)a[c * img + k] - (double)b[c * img + k];
    acc += d * d;
  }
  const double t = block_sum(acc, scratch);
  if (threadIdx.x == 0) unsafeAtomicAdd(&out[c], t);
}

__global__ void axpy_env_kernel(double* f, const double* tvv, const double* sq, int64_t n, float lambda, float gamma) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] -= (double)lambda * (tvv[i] + sq[i] / (2.0 * (double)gamma));
}

hipError_t launch_axpy_env(double* f, const double* tvv, const double* sq, int64_t n, float lambda, float gamma, hipStream_t st) {
  hipLaunchKernelGGL(axpy_env_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, tvv, sq, n, lambda, gamma);
  return hipGetLastError();
}

hipError_t launch_sqdiff(const float* a, const float* b, int64_t n_img, size_t img, double* out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * n_img, st);
  if (e != hipSuccess) return e;
  int gx = (int)((img + 255) / 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(sqdiff_kernel, dim3((unsigned)n_img, gx), dim3(256), 0, st, a, b, img, out);
  return hipGetLastError();
}

}  // namespace lmc
