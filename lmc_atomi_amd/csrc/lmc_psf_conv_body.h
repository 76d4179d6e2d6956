// The body of the large-PSF convolution kernel (lmc_psf_kernel.h), included once per kernel NAME: the including file defines
//   LMC_PSF_KERNEL_HEAD   the template head <int EPI, bool SEP> and the kernel's name, up to its argument list
// Textual inclusion, as lmc_step_tile_kernel.h: psf_conv_kernel keeps its eighteen instantiations and their instruction streams, and the epilogues of the
// Huber data term (kPsfRhoHub, kPsfEnHub) are instantiations of a kernel of their own name, psf_hub_kernel.
LMC_PSF_KERNEL_HEAD(PsfArgs P) {
  __shared__ float xs[kPsfPH * kPsfPW];
  __shared__ float hs[SEP ? kPsfPW2 * kPsfST : 1];
  constexpr bool kEnergy = EPI == kPsfEnL2 || EPI == kPsfEnWl2 || EPI == kPsfEnPois || EPI == kPsfEnHub;
  __shared__ double red[kEnergy ? 4 : 1];
  const int tid = threadIdx.x, tx = tid & (kWave - 1), wv = tid >> 6;
  const int H = P.H, W = P.W;
  const int tiles = P.tiles_x * P.tiles_y;
  const int im = blockIdx.x / tiles, tile = blockIdx.x - im * tiles;       // the image index shares grid.x with the tiles: any number of images
  const int ty0 = (tile / P.tiles_x) * kPsfTH, tx0 = (tile - (tile / P.tiles_x) * P.tiles_x) * kPsfTW;
  const size_t img = (size_t)H * W;
  const float* __restrict__ xi = P.x + (size_t)im * img;
  const int khp = (P.kh + kPsfRows - 1) / kPsfRows * kPsfRows;
  const int rows = kPsfTH + khp - 1;                 // staged rows the window reads; the rows behind kPsfTH + kh - 1 meet zero taps only
  for (int e = tid; e < rows * kPsfPW; e += 256) {
    const int r = e / kPsfPW, c = e - r * kPsfPW;
    const int gr = ty0 + r - P.py, gc = tx0 + c - P.px;
    const bool in = r < kPsfTH + P.kh - 1 && c < kPsfTW + P.kw - 1 && gr >= 0 && gr < H && gc >= 0 && gc < W;
    xs[e] = in ? xi[(size_t)gr * W + gc] : 0.f;
  }
  __syncthreads();
  float acc[kPsfRows];
#pragma unroll
  for (int r = 0; r < kPsfRows; ++r) acc[r] = 0.f;
  const float* __restrict__ g = P.g;
  if constexpr (SEP) {
    const int kwp = (P.kw + kPsfRows - 1) / kPsfRows * kPsfRows;
    const int ncols = kPsfTW + P.kw - 1;             // staged columns that carry data; the row window reads up to kPsfTW + kwp - 1: zeros behind ncols
    for (int e = tid; e < (kPsfTW + kwp - 1 - ncols) * kPsfTH; e += 256) hs[(ncols + e / kPsfTH) * kPsfST + (e & (kPsfTH - 1))] = 0.f;
    for (int c = tx; c < ncols; c += kPsfTW) {       // column factor: hs[c][i] = sum_a gu[a] xs[i + a][c], the lane's 8 rows of column c
      float v[kPsfRows];
#pragma unroll
      for (int r = 0; r < kPsfRows; ++r) v[r] = 0.f;
      psf_column(v, g, xs + wv * kPsfRows * kPsfPW + c, kPsfPW, khp);
#pragma unroll
      for (int r = 0; r < kPsfRows; ++r) hs[c * kPsfST + wv * kPsfRows + r] = v[r];
    }
    __syncthreads();
    const int hr = tid & (kPsfTH - 1), cg = tid >> 5;     // row factor: the lane's row and its 8 columns cg * 8 .. + 7
    float o[kPsfRows];
#pragma unroll
    for (int j = 0; j < kPsfRows; ++j) o[j] = 0.f;
    psf_column(o, g + kPsfKP, hs + cg * kPsfRows * kPsfST + hr, kPsfST, kwp);
#pragma unroll
    for (int j = 0; j < kPsfRows; ++j) xs[hr * kPsfSO + cg * kPsfRows + j] = o[j];      // (every read of the staged tile lies before the barrier above)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kPsfRows; ++r) acc[r] = xs[(wv * kPsfRows + r) * kPsfSO + tx];
  } else {
    for (int b = 0; b < P.kw; ++b) psf_column(acc, g + b * kPsfKP, xs + wv * kPsfRows * kPsfPW + tx + b, kPsfPW, khp);
  }
  const int gc = tx0 + tx;
  double fa = 0.0;
#pragma unroll
  for (int r = 0; r < kPsfRows; ++r) {
    const int gr = ty0 + wv * kPsfRows + r;
    if (gr < H && gc < W) {
      const size_t p = (size_t)gr * W + gc, o = (size_t)im * img + p;
      const float u = acc[r];
      if constexpr (EPI == kPsfRaw) P.out[o] = u;
      if constexpr (EPI == kPsfRhoL2) P.out[o] = u - P.y[p];
      if constexpr (EPI == kPsfRhoWl2) P.out[o] = P.y[img + p] * (u - P.y[p]);
      if constexpr (EPI == kPsfRhoPois) P.out[o] = pois_rho(u, P.y[p], P.y[img + p]);
      if constexpr (EPI == kPsfRhoHub) P.out[o] = hub_psi(u - P.y[p], P.y[img + p]);
      if constexpr (EPI == kPsfSub) P.out[o] = fmaf(-P.coef, u, P.out[o]);
      if constexpr (EPI == kPsfOverwrite) P.out[o] = fmaf(-P.coef, u, P.a * P.xin[o]);
      if constexpr (EPI == kPsfEnL2) { const double d = (double)u - (double)P.y[p]; fa += 0.5 * d * d; }
      if constexpr (EPI == kPsfEnWl2) { const double d = (double)u - (double)P.y[p]; fa += 0.5 * (double)P.y[img + p] * d * d; }
      if constexpr (EPI == kPsfEnPois) fa += pois_phi(u, P.y[p], P.y[img + p]);
      if constexpr (EPI == kPsfEnHub) fa += hub_h(u - P.y[p], P.y[img + p]);
    }
  }
  if constexpr (kEnergy) {      // a fixed order: lanes by shuffles, then the four waves by thread 0 -- no atomics, equal from run to run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) fa += __shfl_down(fa, off, kWave);
    if (tx == 0) red[wv] = fa;
    __syncthreads();
    if (tid == 0) P.part[(size_t)im * tiles + tile] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}
