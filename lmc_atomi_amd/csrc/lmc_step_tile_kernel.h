// The body of the LDS-tiled step kernel (lmc_step_tile.hip), included once per data term: the including file defines
//   LMC_TILE_TERM        the DataTerm of the two kernels
//   LMC_TILE_NAME(sfx)   their names: LMC_TILE_NAME(_kernel)<NP, TV, ANISO> and, by the second pass at the end of this file, LMC_TILE_NAME(_box_kernel)<NP, ANISO>
// Textual inclusion, not a shared device function: the unconstrained kernels keep their instruction streams bit for bit that way (as a
// function inlined into two kernels the same source compiles to other streams for all sixteen -- scripts/kernel_resources.py --code-hash), and the
// box-constrained kernels get names of their own without a fourth template argument on myula_step_tile_kernel.
//
// LDS image: (PH + 2) rows of PW floats; row -1 and row PH are pad rows so that the +-1 neighbour
// reads of tile-border pixels stay inside the allocation (their values never reach the interior:
// information moves one pixel per dual iteration and the halo is >= niter).
// ANISO (with TV): the anisotropic TV prior -- the dual is projected onto the l-infinity unit ball (a clamp per component).
// BOX (with TV; myula_step_tile_box_kernel): the prior is sigma TV + the indicator of [P.box_lo, P.box_hi] -- every primal iterate, the returned one
// included, is projected onto the box (Beck and Teboulle's constrained FGP).  Pixels outside the image then hold the clamp of 0; the has-down / has-right
// flags cut every difference with them, and their own dual stays 0 (no flag set), as before.
// TERM == kTermPois (myula_step_tile_pois_kernel, myula_step_tile_pois_box_kernel): the Poisson data term -- P.y is [2][H][W], counts then background, and the
// residual H x - y becomes rho(H x) = phi'(H x) (pois_rho, lmc_device.h) at the three places that form it.  P.data_kind stays the operator's kind.
// TERM == kTermWl2 (myula_step_tile_wl2_kernel, myula_step_tile_wl2_box_kernel): the weighted Gaussian data term -- P.y is [2][H][W], observation then weights, and
// the residual H x - y becomes w (H x - y): the weight multiplies BEFORE the adjoint.  Identity and blur (there is no weighted mask kind).
// TERM == kTermHub (myula_step_tile_hub_kernel, myula_step_tile_hub_box_kernel): the Huber data term -- P.y is [2][H][W], observation then thresholds delta, and the
// residual H x - y becomes clamp(H x - y, -delta, delta) (hub_psi, lmc_device.h): the clamp acts BEFORE the adjoint.  Identity and blur (no mask kind).
#ifndef LMC_TILE_BOX_PASS
template <int NP, bool TV, bool ANISO = false> __global__ __launch_bounds__(kStepThreads) void LMC_TILE_NAME(_kernel)(const StepArgs P) {
  constexpr bool BOX = false;
#else
template <int NP, bool ANISO> __global__ __launch_bounds__(kStepThreads) void LMC_TILE_NAME(_box_kernel)(const StepArgs P) {
  constexpr bool TV = true, BOX = true;
#endif
  constexpr int TERM = LMC_TILE_TERM;
  static_assert(TV || !ANISO, "the anisotropic projection belongs to the TV prox");
  static_assert(TV || !BOX, "the box is part of the TV prox here (separable priors: box_prior_prox_kernel)");
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int logical = xcd_logical_block(blockIdx.x, gridDim.x);
  const int tiles = P.tiles_x * P.tiles_y;
  const int chain = logical / tiles;
  const int tile = logical - chain * tiles;
  const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
  const int H = P.H, W = P.W, PW = P.PW, PH = P.PH, HL = P.HL;
  const int row0 = ty * P.TH - HL, col0 = tx * P.TW - HL;  // image coords of tile pixel (0,0)
  const int npix = PH * PW;
  const int arr = (PH + 2) * PW;
  float* xs = lds + PW;   // x tile (+halo), zero outside the image
  float* S = xs + arr;    // blur residual, then TV primal iterate ("sol")
  float* A = S + arr;     // dual, row component    (TV only)
  float* B = A + arr;     // dual, column component (TV only)

  const size_t img = (size_t)H * W;
  const float* __restrict__ xin = P.x_in + (size_t)chain * img;

  // ---- phase 0: stage x tile; each thread owns pixels p = tid + m*1024 -------------------
  float xv[NP];
  int flags[NP];  // bit0 in image, bit1 has-down, bit2 has-right, bit3 p < npix
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    const int p = tid + m * kStepThreads;
    float v = 0.f;
    int f = 0;
    if (p < npix) {
      const int r = p / PW, c = p - r * PW;
      const int gr = row0 + r, gc = col0 + c;
      const bool in = (gr >= 0) & (gr < H) & (gc >= 0) & (gc < W);
      if (in) v = xin[(size_t)gr * W + gc];
      f = 8 | (in ? 1 : 0) | ((in && gr + 1 < H) ? 2 : 0) | ((in && gc + 1 < W) ? 4 : 0);
      xs[p] = v;
      if (TV) { A[p] = 0.f; B[p] = 0.f; }
    }
    xv[m] = v;
    flags[m] = f;
  }
  if (TV) {  // zero the pad rows of the dual arrays
    for (int i = tid; i < PW; i += kStepThreads) {
      A[-PW + i] = 0.f; B[-PW + i] = 0.f; A[npix + i] = 0.f; B[npix + i] = 0.f;
      S[-PW + i] = 0.f; S[npix + i] = 0.f;
    }
  }
  __syncthreads();

  // interior ownership for gradient / combine: thread -> column ci, rows 4*rg .. 4*rg+3
  const int ci = tid % P.TW, rg = tid / P.TW;
  const bool own_int = rg < (P.TH >> 2);
  float gv[4] = {0.f, 0.f, 0.f, 0.f};

  // ---- phase 1+2: grad f = sigma_f * H^T (H x - y) ----------------------------------------
  if (P.data_kind == LMC_DATA_BLUR) {
    const int kh = P.blur.kh, kw = P.blur.kw, oy = P.blur.oy, ox = P.blur.ox;
    const int r_lo = HL - oy, r_hi = HL + P.TH + kh - 1 - oy;  // rows of R needed by H^T
    const int c_lo = HL - ox, c_hi = HL + P.TW + kw - 1 - ox;
#pragma unroll
    for (int m = 0; m < NP; ++m) {
      const int p = tid + m * kStepThreads;
      if (p < npix) {
        const int r = p / PW, c = p - r * PW;
        if (r >= r_lo && r < r_hi && c >= c_lo && c < c_hi) {
          float acc = 0.f;
          if (flags[m] & 1) {
            for (int a = 0; a < kh; ++a)
              for (int b = 0; b < kw; ++b)
                acc = fmaf(P.blur.h[a * kw + b], xs[(r - a + oy) * PW + (c - b + ox)], acc);
            const size_t gi = (size_t)(row0 + r) * W + (col0 + c);
            // (inside the guard: rho of a pixel outside the image is not 0 -- it is 1 for y = 0)
            if constexpr (TERM == kTermPois) acc = pois_rho(acc, P.y[gi], P.y[img + gi]);
            else if constexpr (TERM == kTermWl2) acc = P.y[img + gi] * (acc - P.y[gi]);
            else if constexpr (TERM == kTermHub) acc = hub_psi(acc - P.y[gi], P.y[img + gi]);
            else acc -= P.y[gi];
          }
          S[p] = acc;  // residual, zero outside the image (zero-padded adjoint)
        }
      }
    }
    __syncthreads();
    if (own_int) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = HL + 4 * rg + j, c = HL + ci;
        float acc = 0.f;
        for (int a = 0; a < kh; ++a)
          for (int b = 0; b < kw; ++b)
            acc = fmaf(P.blur.h[a * kw + b], S[(r + a - oy) * PW + (c + b - ox)], acc);
        gv[j] = P.sigma_f * acc;
      }
    }
    __syncthreads();
  }

  // ---- phase 3: TV prox, K fast-gradient-projection dual iterations -----------------------
  if (TV) {
    float rrv[NP], ssv[NP], pv[NP], qv[NP], solv[NP];
#pragma unroll
    for (int m = 0; m < NP; ++m) { rrv[m] = ssv[m] = pv[m] = qv[m] = 0.f; }
    if (P.tv_in) {   // resume: dual state of the previous launch (tile + halo), zero outside the image
      const float* __restrict__ st = P.tv_in + (size_t)chain * 4 * img;
#pragma unroll
      for (int m = 0; m < NP; ++m) {
        const int p = tid + m * kStepThreads;
        if (p < npix && (flags[m] & 1)) {
          const int r = p / PW, c = p - r * PW;
          const size_t gi = (size_t)(row0 + r) * W + (col0 + c);
          rrv[m] = st[gi]; ssv[m] = st[img + gi]; pv[m] = st[2 * img + gi]; qv[m] = st[3 * img + gi];
          A[p] = rrv[m]; B[p] = ssv[m];
        }
      }
      __syncthreads();
    }
    const float gam = P.tv.gamma, cstep = P.tv.c;
    for (int k = 0; k <= P.tv.niter; ++k) {
      // A-phase: sol = x - gamma * div(rr, ss)
#pragma unroll
      for (int m = 0; m < NP; ++m) {
        const int p = tid + m * kStepThreads;
        if (p < npix) {
          const float dv = (rrv[m] - A[p - PW]) + (ssv[m] - B[p - 1]);
          solv[m] = fmaf(-gam, dv, xv[m]);
          if constexpr (BOX) solv[m] = __builtin_amdgcn_fmed3f(solv[m], P.box_lo, P.box_hi);
          S[p] = solv[m];
        }
      }
      __syncthreads();
      if (k == P.tv.niter) break;
      const float beta = P.tv.betas[k];
      // B-phase: dual ascent step, projection onto the unit ball, momentum
#pragma unroll
      for (int m = 0; m < NP; ++m) {
        const int p = tid + m * kStepThreads;
        if (p < npix) {
          const float dx = (flags[m] & 2) ? S[p + PW] - solv[m] : 0.f;
          const float dy = (flags[m] & 4) ? S[p + 1] - solv[m] : 0.f;
          const float r = fmaf(-cstep, dx, rrv[m]);
          const float s = fmaf(-cstep, dy, ssv[m]);
          float pn, qn;
          if constexpr (ANISO) {
            pn = __builtin_amdgcn_fmed3f(r, -1.f, 1.f);
            qn = __builtin_amdgcn_fmed3f(s, -1.f, 1.f);
          } else {
            const float inv = rsqrtf(fmaxf(fmaf(r, r, s * s), 1.f));
            pn = r * inv; qn = s * inv;
          }
          rrv[m] = fmaf(beta, pn - pv[m], pn);
          ssv[m] = fmaf(beta, qn - qv[m], qn);
          pv[m] = pn;
          qv[m] = qn;
          A[p] = rrv[m];
          B[p] = ssv[m];
        }
      }
      __syncthreads();
    }
    if (P.tv_out) {   // store the dual state of the tile interior for the next launch
      float* __restrict__ st = P.tv_out + (size_t)chain * 4 * img;
#pragma unroll
      for (int m = 0; m < NP; ++m) {
        const int p = tid + m * kStepThreads;
        if (p < npix && (flags[m] & 1)) {
          const int r = p / PW, c = p - r * PW;
          if (r >= HL && r < HL + P.TH && c >= HL && c < HL + P.TW) {
            const size_t gi = (size_t)(row0 + r) * W + (col0 + c);
            st[gi] = rrv[m]; st[img + gi] = ssv[m]; st[2 * img + gi] = pv[m]; st[3 * img + gi] = qv[m];
          }
        }
      }
    }
  }
  if (P.tv_state_only) return;

  // ---- phase 4: combine + noise + store ----------------------------------------------------
  if (!own_int) return;
  const int gc = col0 + HL + ci;
  const int gr0 = row0 + HL + 4 * rg;
  if (gc >= W || gr0 >= H) return;
  float xi[4] = {0.f, 0.f, 0.f, 0.f};
  if (P.noise_mode == LMC_NOISE_PHILOX) {
    // gr0 is a multiple of 4 because TH is: the quad of rows gr0..gr0+3
    quad_normals(P.key0, P.key1, P.iteration, P.chain_offset + (uint32_t)chain,
                 (uint32_t)(gr0 >> 2) * (uint32_t)W + (uint32_t)gc, xi);
  }
  float* __restrict__ xout = P.x_out + (size_t)chain * img;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gr = gr0 + j;
    if (gr >= H) break;
    const int p = (HL + 4 * rg + j) * PW + HL + ci;
    const size_t gi = (size_t)gr * W + gc;
    const float x = xs[p];
    float g = gv[j];
    if (P.data_kind == LMC_DATA_IDENTITY) {
      if constexpr (TERM == kTermPois) g = P.sigma_f * pois_rho(x, P.y[gi], P.y[img + gi]);
      else if constexpr (TERM == kTermWl2) g = P.sigma_f * (P.y[img + gi] * (x - P.y[gi]));
      else if constexpr (TERM == kTermHub) g = P.sigma_f * hub_psi(x - P.y[gi], P.y[img + gi]);
      else g = P.sigma_f * (x - P.y[gi]);
    } else if (P.data_kind == LMC_DATA_MASK) {
      const float mk = P.mask[gi];
      if constexpr (TERM == kTermPois) g = P.sigma_f * mk * pois_rho(mk * x, P.y[gi], P.y[img + gi]);
      else g = P.sigma_f * mk * fmaf(mk, x, -P.y[gi]);
    }
    if (P.ncvx_kind == LMC_NCVX_MC_TV) {   // - lambda * A^T(A x / max(|A x|, gamma))  (algs.py:273-277, 291)
      g -= P.ncvx_lambda * mc_tv_grad(xs[p - PW], xs[p - PW + 1], xs[p - 1], x, xs[p + 1], xs[p + PW - 1], xs[p + PW],
                                      gr > 0, gr + 1 < H, gc > 0, gc + 1 < W, P.ncvx_gamma);
    }
    if (P.extra) g = fmaf(P.extra_coef, x - P.extra[(size_t)chain * img + gi], g);   // ME-TV: -lambda/gamma (x - prox_{gamma TV}(x))
    float px;
    if (TV) {
      px = S[p];
    } else if (P.prior_kind == LMC_PRIOR_L2) {
      px = x * P.prior_p0;
    } else if (P.prior_kind == LMC_PRIOR_L1) {
      px = copysignf(fmaxf(fabsf(x) - P.prior_p0, 0.f), x);
    } else {
      px = x;
    }
    if (P.prox_ext) px = P.prox_ext[(size_t)chain * img + gi];
    float nz = xi[j];
    if (P.noise_mode == LMC_NOISE_INJECTED) nz = P.noise[(size_t)chain * img + gi];
    xout[gi] = fmaf(P.a, x, fmaf(-P.t, g, fmaf(P.b, px, P.s * nz)));
  }
}
#ifndef LMC_TILE_BOX_PASS
#define LMC_TILE_BOX_PASS
#include "lmc_step_tile_kernel.h"
#undef LMC_TILE_BOX_PASS
#endif
