// FGP momentum folded into the projection scale (pipe_stage<..., FOLD>, lmc_step_pipe_kernel.h): the two coefficients a stage reads instead of beta_k.
// A stage hands on u_k = (1 + beta_k) p_k in place of the projected dual p_k, so the extrapolated dual is
//     rr_k = p_k + beta_k (p_k - p_{k-1}) = u_k - c_k u_{k-1},      c_k = beta_k / (1 + beta_{k-1}),   c_1 = 0  (p_0 = 0: stage 1 reads no u_0).
// Plain C++, no device code: formed in double from the float table the kernels would read, rounded once.  beta = 0 (momentum off) gives 1 and 0.
#pragma once

namespace lmc {

constexpr int kTvFoldMax = 10;        // stages of one pipe launch at most

// tab[2 k] = 1 + beta_{k+1}, tab[2 k + 1] = c_{k+1} for k = 0 .. n - 1 (n <= kTvFoldMax).  False: some beta_k is -1 or not finite (no momentum
// sequence in use comes near: beta_k is in [0, 1)), so u_k would not determine p_k; the table is then not to be used.
inline bool tv_fold_table(const float* betas, int n, float* tab) {
  double prev = 0.0;
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    const double b = (double)betas[k];
    ok = ok && 1.0 + b != 0.0 && b > -3.0e38 && b < 3.0e38;
    tab[2 * k] = (float)(1.0 + b);
    tab[2 * k + 1] = k == 0 ? 0.f : (float)(b / (1.0 + prev));
    prev = b;
  }
  return ok;
}

}  // namespace lmc
