// The SAPG update of the prior weight (definition: include/lmc_atomi.h), one inline function for the host entry point lmc_sapg_update and
// for sapg_update_kernel: both compile from it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace lmc {

struct SapgParams {
  double dim_eff, degree;              // d, k
  double step_scale, step_exponent;    // c0, p
  double theta_min, theta_max;
};

// theta_{n+1} from theta_n and gbar, n the 0-based update index.  A step that leaves [theta_min, theta_max] returns the bound itself
// (not exp(log(bound))); a NaN gbar gives NaN, which the caller refuses.
__host__ __device__ inline double sapg_next_theta(const SapgParams& P, long long n, double theta, double gbar) {
  const double delta = P.step_scale * pow((double)(n + 1), -P.step_exponent) / P.dim_eff;
  const double eta = log(theta) + delta * (P.dim_eff / P.degree - theta * gbar);
  if (eta <= log(P.theta_min)) return P.theta_min;
  if (eta >= log(P.theta_max)) return P.theta_max;
  return exp(eta);
}

}  // namespace lmc
