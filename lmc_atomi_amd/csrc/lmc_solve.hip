// The implicit step of ULPDA and lmc_l2_prox: (I + ts H^T H) u = rhs for every chain, by Chebyshev semi-iteration where it covers the problem,
// else by conjugate gradients.
#include <cmath>
#include <cstring>
#include <vector>

#include "lmc_host.h"

namespace lmc::host {

// Conjugate gradients on (I + ts H^T H) u = rhs for every chain, `niter` iterations from the current u.
// The operator q = p + ts H^T H p is ONE launch of the fused step kernel (out = 1*p - t*grad f(p) with y = 0 and
// t = -ts/sigma_f), i.e. the same blur pipeline as the sampler; zero_y is an all-zero [H][W] image.
// scal: 4C + 1 doubles (rs, pq, rs_new, |rhs|^2 per chain, and the "converged" flag).
// Chebyshev semi-iteration for (I + ts H^T H) u = rhs.  The spectrum is known: H^T H lies in [0, (sum |h|)^2] (zero-padded
// convolution, Young's inequality), so A lies in [1, 1 + ts (sum |h|)^2] and the three-term recurrence (Saad, Iterative Methods,
// alg. 12.1)   u_{k+1} = u_k + alpha_k (rhs - A u_k) + beta_k (u_k - u_{k-1})   needs no inner products at all.  One iteration is ONE
// launch of the row-streaming step kernel:  out = a x - t sigma_f H^T H x + b ext + s prev  with x = u_k, ext = rhs, prev = u_{k-1} read
// through the injected-noise input and overwritten in place by u_{k+1} (pointwise read-then-write by the same lane): 16 B per pixel
// and iteration instead of the 44 B and six launches of a CG iteration.  The residual of the k-th iterate is max|p_k| |r_0| with
// max|p_k| <= 2 c^k, c = (sqrt(kappa) - 1) / (sqrt(kappa) + 1): the iteration count for the reference's stopping rule |r| <= tol |b|
// (scipy lsqr btol, algs.py:250) is known in advance -- no convergence test, no flags, no host synchronisation.
// Returns hipErrorInvalidConfiguration when the row-streaming kernel does not cover the problem (caller falls back to CG).
// pb (optional): two scratch arrays and the array that receives the solution, all [C][H][W] and distinct from u / tmp / rhs.  With them, and
// where lmc_cheb_pair.hip covers the problem, the iterations after the first run TWO per launch (20 instead of 32 B per pixel); the solution
// then arrives in pb->out, u (the starting guess) is used as scratch, and *result says which of the two holds it.
struct ChebPairBufs { float* b1; float* b2; float* out; };
static hipError_t chebyshev_solve(const Problem& q, float ts, float* u, const float* rhs, float* tmp, double* scal, int64_t C, int niter_cap,
                                  float tol, const float* zero_y, hipStream_t st, const ChebPairBufs* pb = nullptr, float** result = nullptr) {
  if (result) *result = u;
  lmc::StepArgs A;
  std::memset(&A, 0, sizeof A);
  A.H = q.H; A.W = q.W; A.C = (int)C;
  A.data_kind = LMC_DATA_BLUR; A.sigma_f = q.sigma_f; A.blur = q.taps;
  A.y = zero_y; A.mask = zero_y;
  A.prior_kind = LMC_PRIOR_NONE;
  A.prox_ext = rhs;
  A.noise = zero_y;
  A.noise_mode = LMC_NOISE_NONE;
  A.x_in = u; A.x_out = tmp;
  if (!lmc::rows_supported(A)) return hipErrorInvalidConfiguration;
  double hsum = 0.0;
  for (int i = 0; i < q.taps.kh * q.taps.kw; ++i) hsum += std::fabs((double)q.taps.h[i]);
  const double lmin = 1.0, lmax = 1.0 + (double)ts * hsum * hsum * 1.0001;       // a hair of slack for the fp32 taps
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  int k_need = 1;
  if (delta > 1e-12 * theta) {
    const double sk = std::sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
    k_need = (int)std::ceil(std::log(2.0 / (double)tol) / std::log(1.0 / c)) + 1;   // +1: a warm start may begin with |r_0| > |b|
  }
  // A cap below what the tolerance needs makes the answer depend on the solver (a truncated iterate): leave that case to CG, whose
  // truncated iterates are the ones pinned by the tests; here every solve reaches the tolerance.
  if (k_need > niter_cap) return hipErrorInvalidConfiguration;
  int K = k_need;
  // A warm start begins with |r_0| << |rhs|: the first launch measures |r_0| and |rhs| on the fly, a one-block kernel turns them into the
  // number of launches needed (even, <= the a-priori count), and the launches beyond it return at their first instruction.
  // (the adaptive count is even; when rounding up would exceed the caller's cap the a-priori count runs as it is)
  const bool adaptive = K > 2 && delta > 1e-12 * theta && ((K + 1) & ~1) <= niter_cap;
  if (adaptive) {
    K = (K + 1) & ~1;
    hipError_t e = hipMemsetAsync(scal, 0, sizeof(double) * (4 * C + 1), st);
    if (e != hipSuccess) return e;
  }
  const size_t img = (size_t)q.H * q.W;
  // lmc_problem.iterations_per_launch / LMC_CHEB_PAIR (resolved when the problem is loaded: sampler creation, or the stateless call): 0 = single-iteration
  // launches only, 2 = pairs wherever the kernel covers the problem (tests), default = where they pay
  const int pair_mode = q.cheb_pair;
  const bool pair_on = pair_mode == 2 || (pair_mode == 1 && lmc::cheb_pair_pays(C, q.H));
  if (pb && result && pair_on && K >= 4 && 2 * ((K + 1) / 2) <= niter_cap && delta > 1e-12 * theta &&
      lmc::cheb_pair_supported(q.H, q.W, q.taps)) {      // (pairs never run more iterations than the caller's cap)
    // pairs p = 1 .. M of iterations 2p - 2, 2p - 1.  The first one also forms the residual statistics of iteration 0 (the adaptive count, known
    // after it); the second always runs (the solution has to arrive in pb->out, and the first cannot know whether it is the last); pair p >= 3
    // returns at once when count <= 2p - 2; the last pair that runs writes to pb->out.
    const int M = (K + 1) / 2;
    const int n_it = 2 * M;
    std::vector<double> al(n_it), be(n_it);
    {
      double rho = delta / theta;
      const double sigma1 = theta / delta;
      al[0] = 1.0 / theta; be[0] = 0.0;
      for (int k = 1; k < n_it; ++k) {
        const double rho_new = 1.0 / (2.0 * sigma1 - rho);
        al[k] = 2.0 * rho_new / delta;
        be[k] = rho_new * rho;
        rho = rho_new;
      }
    }
    double* stat = scal;
    int* count = reinterpret_cast<int*>(scal + 4 * C);
    const float* cur = u;
    const float* prv = u;          // iteration 0 has no u_{-1} (s0 = 0): any valid array
    float* f1 = tmp;
    float* f2 = pb->b1;
    float* spare = pb->b2;
    for (int p = 1; p <= M; ++p) {
      const int k0 = 2 * p - 2, k1 = 2 * p - 1;
      lmc::ChebPairArgs P;
      std::memset(&P, 0, sizeof P);
      P.H = q.H; P.W = q.W; P.C = (int)C;
      P.cur = cur; P.prv = prv; P.rhs = rhs; P.f1 = f1; P.f2 = f2; P.f2_last = p == 1 ? f2 : pb->out;
      P.a0 = (float)(1.0 - al[k0] + be[k0]); P.tg0 = (float)(al[k0] * (double)ts); P.b0 = (float)al[k0]; P.s0 = (float)(-be[k0]);
      P.a1 = (float)(1.0 - al[k1] + be[k1]); P.tg1 = (float)(al[k1] * (double)ts); P.b1 = (float)al[k1]; P.s1 = (float)(-be[k1]);
      P.run_count = adaptive && p >= 2 ? count : nullptr;
      P.run_index = p <= 2 ? -1 : k0;           // *count <= k0: iterations k0, k0 + 1 are not needed
      P.last_index = k1 + 1;                    // no later pair runs when *count <= 2p
      P.force_last = p == M;
      P.dot_out = adaptive && p == 1 ? stat : nullptr;
      hipError_t e = lmc::launch_cheb_pair(P, q.taps, st);
      if (e != hipSuccess) return e;
      if (adaptive && p == 1) {
        const double sk = std::sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
        e = lmc::cheb_count(C, stat, 1.0 / ((double)P.b0 * (double)P.b0), (double)tol, 1.0 / std::log(1.0 / c), 2 * M, count, st);
        if (e != hipSuccess) return e;
      }
      // u_{k+2} = f2 and u_{k+1} = f1 are the next pair's inputs; the arrays it read are free again (u itself from the second pair on)
      float* free_a = p == 1 ? spare : const_cast<float*>(cur);
      float* free_b = p == 1 ? u : const_cast<float*>(prv);
      cur = f2; prv = f1; f1 = free_a; f2 = free_b;
    }
    *result = pb->out;
    return hipSuccess;
  }
  double* stat = scal;                                    // [2C]
  int* count = reinterpret_cast<int*>(scal + 2 * C);      // the solver's flag word (the second [2C] block is free here)
  float* cur = u;
  float* oth = tmp;
  double rho = delta > 0 ? delta / theta : 0.0;      // rho_0 = 1 / sigma_1
  const double sigma1 = delta > 0 ? theta / delta : 0.0;
  for (int k = 0; k < K; ++k) {
    double alpha, beta;
    if (k == 0 || !(delta > 1e-12 * theta)) { alpha = 1.0 / theta; beta = 0.0; }
    else {
      const double rho_new = 1.0 / (2.0 * sigma1 - rho);
      alpha = 2.0 * rho_new / delta;
      beta = rho_new * rho;
      rho = rho_new;
    }
    A.x_in = cur; A.x_out = oth;
    A.a = (float)(1.0 - alpha + beta);
    A.t = (float)(alpha * (double)ts / (double)q.sigma_f);
    A.b = (float)alpha;
    if (beta != 0.0) { A.noise_mode = LMC_NOISE_INJECTED; A.noise = oth; A.s = (float)(-beta); }   // oth holds u_{k-1} and receives u_{k+1}
    else { A.noise_mode = LMC_NOISE_NONE; A.noise = zero_y; A.s = 0.f; }
    A.dot_out = nullptr; A.dot_mode = 0; A.run_count = nullptr; A.run_index = 0;
    if (adaptive) {
      if (k == 0) { A.dot_out = stat; A.dot_mode = 1; }
      else { A.run_count = count; A.run_index = k; }
    }
    hipError_t e = lmc::launch_step_rows(A, st);
    if (e != hipSuccess) return e;
    if (adaptive && k == 0) {
      const double sk = std::sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
      e = lmc::cheb_count(C, stat, 1.0 / ((double)A.b * (double)A.b), (double)tol, 1.0 / std::log(1.0 / c), K, count, st);
      if (e != hipSuccess) return e;
    }
    float* t = cur; cur = oth; oth = t;
  }
  if (cur != u) return hipMemcpyAsync(u, cur, sizeof(float) * (size_t)C * img, hipMemcpyDeviceToDevice, st);
  return hipSuccess;
}

// alt_out / result (optional, both or none): an extra [C][H][W] array the solution may arrive in instead of u (*result tells); u is then scratch.
int cg_solve_fused(const Problem& q, float ts, float* u, const float* rhs, float* r, float* p, float* qq, double* scal,
                   int64_t C, int niter, const float* zero_y, hipStream_t st, float* alt_out, float** result) {
  if (result) *result = u;
  const size_t img = (size_t)q.H * q.W;
  const float cg_tol = tol_of(q);
  if (cg_tol > 0.f) {     // Chebyshev whenever a tolerance is set and it covers the problem; CG for everything else
    const ChebPairBufs pb{p, qq, alt_out};
    hipError_t e = chebyshev_solve(q, ts, u, rhs, r, scal, C, niter, cg_tol, zero_y, st, alt_out && result ? &pb : nullptr, result);
    if (e == hipSuccess) return LMC_OK;
    if (e != hipErrorInvalidConfiguration) HIP_TRY(e);
  }
  double *rs = scal, *pq = scal + C, *rs_new = scal + 2 * C, *b2 = scal + 3 * C;
  int* done = reinterpret_cast<int*>(scal + 4 * C);
  const bool early = cg_tol > 0.f;
  const double tol2 = (double)cg_tol * (double)cg_tol;
  lmc::StepArgs A;
  std::memset(&A, 0, sizeof A);
  A.H = q.H; A.W = q.W; A.C = (int)C;
  A.data_kind = LMC_DATA_BLUR; A.sigma_f = q.sigma_f; A.blur = q.taps;
  A.y = zero_y; A.mask = zero_y; A.noise = zero_y;
  A.prior_kind = LMC_PRIOR_NONE;
  A.a = 1.f; A.t = -ts / q.sigma_f; A.b = 0.f; A.s = 0.f;
  A.noise_mode = LMC_NOISE_NONE;
  const char* kname = nullptr;
  Workspace none;      // (a blur without a prior: the launch takes no work buffer)
  auto apply = [&](const float* in, float* out) -> hipError_t { A.x_in = in; A.x_out = out; return launch_step(A, q, none, st, &kname); };
  HIP_TRY(hipMemsetAsync(scal, 0, sizeof(double) * (4 * C + 1), st));
  HIP_TRY(apply(u, qq));
  A.dot_out = pq;            // the row-streaming kernel accumulates p.Ap while it writes Ap (one pass less per iteration)
  if (early) A.skip_flag = done;
  HIP_TRY(lmc::cg_init(rhs, qq, r, p, C, img, rs, b2, st));
  // Stopping rule = the reference's: its solver (scipy lsqr, algs.py:250) ends at |r| <= btol |b| with btol = 1e-6 by default,
  // or after niter iterations.  Here: when EVERY chain of the batch satisfies it.  The test runs on the device; once the flag is
  // set the kernels of the remaining iterations return at their first instruction (no host synchronisation anywhere).
  if (early) HIP_TRY(lmc::cg_check(C, rs, b2, tol2, done, st));
  for (int it = 0; it < niter; ++it) {
    HIP_TRY(hipMemsetAsync(pq, 0, sizeof(double) * 2 * C, st));     // pq and rs_new are adjacent
    HIP_TRY(apply(p, qq));
    if (!kname || std::strcmp(kname, "myula_step_rows_kernel") != 0) HIP_TRY(lmc::cg_dot(p, qq, C, img, pq, early ? done : nullptr, st));
    HIP_TRY(lmc::cg_update(u, r, p, qq, C, img, rs, pq, rs_new, early ? done : nullptr, st));
    if (early) HIP_TRY(lmc::cg_check(C, rs_new, b2, tol2, done, st));
    HIP_TRY(lmc::cg_dir(p, r, C, img, rs, rs_new, early ? done : nullptr, st));
    HIP_TRY(hipMemcpyAsync(rs, rs_new, sizeof(double) * C, hipMemcpyDeviceToDevice, st));
  }
  return LMC_OK;
}

}  // namespace lmc::host
