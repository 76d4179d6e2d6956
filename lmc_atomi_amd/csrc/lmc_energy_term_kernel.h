// The body of the energy kernel of a data term with a second plane of y (lmc_ops.hip), included once per term: the including file defines
//   LMC_ENERGY_TERM          the DataTerm
//   LMC_ENERGY_TERM_KERNEL   the kernel's name
// Textual inclusion, not a shared device function, as in lmc_step_tile_kernel.h: inlined from a function template the same source compiles to other
// instruction streams (the block size is read another way and the argument loads are scheduled in another order -- scripts/kernel_resources.py --code-hash).
//
// f_out[i] += sigma_f sum_p phi_p((Op x_i)_p), u = Op x in fp32 with the operator's arithmetic of energy_kernel, phi widened to and summed in float64, a
// plain reduction at every width.  E.data_kind is the operator's kind (identity or blur; the mask for Poisson alone: the branch is compiled for that term
// only), E.y the first plane and E.y + H W the second:
//   kTermPois  counts, background: phi = pois_phi
//   kTermWl2   observation, weights: phi = w (u - y)^2 / 2, the half applied once to the block's sum
//   kTermHub   observation, thresholds: phi = hub_h of the residual r = u - y in fp32 (the operand the step kernels clamp; lmc_device.h).  delta = 0 takes the
//              linear branch, which gives 0; delta = +inf the quadratic one, so no inf * 0 is formed
__global__ __launch_bounds__(256) void LMC_ENERGY_TERM_KERNEL(const float* __restrict__ x, EnergyArgs E, double* __restrict__ f_out) {
  constexpr int TERM = LMC_ENERGY_TERM;
  __shared__ double scratch[4];
  const int H = E.H, W = E.W;
  const size_t img = (size_t)H * W;
  const float* xi = x + (size_t)blockIdx.y * img;
  double fa = 0.0;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < img; p += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(p / W), c = (int)(p - (size_t)r * W);
    float u = xi[p];
    if (E.data_kind == LMC_DATA_BLUR) {
      float acc = 0.f;
      for (int a = 0; a < E.blur.kh; ++a)
        for (int b = 0; b < E.blur.kw; ++b) {
          const int rr = r - a + E.blur.oy, cc = c - b + E.blur.ox;
          if (rr >= 0 && rr < H && cc >= 0 && cc < W) acc = fmaf(E.blur.h[a * E.blur.kw + b], xi[(size_t)rr * W + cc], acc);
        }
      u = acc;
    } else if (TERM == kTermPois && E.data_kind == LMC_DATA_MASK) {
      u = E.mask[p] * u;
    }
    if constexpr (TERM == kTermPois) fa += pois_phi(u, E.y[p], E.y[img + p]);
    if constexpr (TERM == kTermWl2) { const double d = (double)u - (double)E.y[p]; fa += (double)E.y[img + p] * d * d; }
    if constexpr (TERM == kTermHub) fa += hub_h(u - E.y[p], E.y[img + p]);
  }
  const double ft = block_sum(fa, scratch);
  if (threadIdx.x == 0) unsafeAtomicAdd(&f_out[blockIdx.y], (TERM == kTermWl2 ? 0.5 * (double)E.sigma_f : (double)E.sigma_f) * ft);
}
