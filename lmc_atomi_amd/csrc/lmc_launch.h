// Host-side launcher declarations (defined in lmc_step_*.hip / lmc_ops.hip).
#pragma once
#include "lmc_common.h"

namespace lmc {

struct EnergyArgs {
  int H, W;
  int data_kind;
  float sigma_f;
  const float* y;
  const float* mask;
  BlurTaps blur;
  int prior_kind;
  float prior_sigma;
  int ncvx_kind;          // f -= ncvx_lambda * sum huber_gamma(|grad x|)  (algs.py:173-190, MC-TV isotropic)
  float ncvx_lambda, ncvx_gamma;
};

hipError_t launch_step_tile(StepArgs a, hipStream_t st);
bool tile_needs_chunks(const StepArgs& a);
hipError_t launch_step_tile_chunked(const StepArgs& a, float* state0, float* state1, hipStream_t st);
hipError_t launch_axpy_env(double* f, const double* tvv, const double* sq, int64_t n, float lambda, float gamma, hipStream_t st);
hipError_t launch_sqdiff(const float* a, const float* b, int64_t n_img, size_t img, double* out, hipStream_t st);
hipError_t launch_blur(const float* x, float* out, int64_t n_img, int H, int W, const BlurTaps& T, int adjoint,
                       hipStream_t st);
hipError_t launch_gradient(const float* x, float* out, int64_t n_img, int H, int W, bool adjoint, hipStream_t st);
hipError_t launch_dual_project(const float* y, float* out, int64_t n_img, int H, int W, float radius, int iso,
                               hipStream_t st);
hipError_t launch_eprox(int kind, const float* x, float* out, int64_t n, float p0, float p1, hipStream_t st);
hipError_t launch_prior_prox_scaled(int prior, int kind, const float* x, float* out, int64_t n_chains, int64_t img, const float* scale, int64_t cs, int64_t ps,
                                    float pt, float sigma, float p0, float p1, int mask, hipStream_t st);
// clip(prox_{t g}(x), lo, hi) for the separable priors (none, l2, l1, EPROX), lmc_box.hip: scale == NULL -- p0 / p1 are the step's parameters (StepArgs::prior_p0 /
// prior_p1); scale != NULL -- array-valued prox parameter, the arguments of launch_prior_prox_scaled
hipError_t launch_box_prox(int prior, int kind, const float* x, float* out, int64_t n_chains, int64_t img, const float* scale, int64_t cs, int64_t ps,
                           float pt, float sigma, float p0, float p1, int mask, float lo, float hi, hipStream_t st);
hipError_t launch_haar_prox(const float* x, float* out, int64_t n_img, int H, int W, float thr, hipStream_t st);
hipError_t launch_chain_probes(const float* x, float* out, int64_t n_img, int H, int W, int ph, int pw, hipStream_t st);
hipError_t launch_haar_value(const float* x, int64_t n_img, int H, int W, float sigma, double* val, hipStream_t st);
hipError_t launch_mc_tv_add(const float* x, float* out, int64_t n_img, int H, int W, float coef, float gamma, hipStream_t st);
hipError_t launch_moments(const float* x, int C, int H, int W, double* s1, double* s2, hipStream_t st);
hipError_t launch_moments_bg(const float* x, int C, int H, int W, double* s1, double* s2, int n_wg, hipStream_t st);
// multi-scale moments (lmc_moments_ms.hip): the pixel accumulators and sum b^2 of the block sums b of every enabled scale, in one pass
struct BlockScales {
  double* s2[4];          // by scale 2, 4, 8, 16: [ceil(H / s)][ceil(W / s)] doubles, NULL = that scale is off
};
hipError_t launch_moments_ms(const float* x, int C, int H, int W, double* s1, double* s2, const BlockScales& B, hipStream_t st);
hipError_t launch_moments_ms_bg(const float* x, int C, int H, int W, double* s1, double* s2, const BlockScales& B, int n_wg, hipStream_t st);
hipError_t launch_block_sums(const double* src, int H, int W, int scale, double* out, hipStream_t st);
// pixel-wise histograms (lmc_pixel_hist.hip): counts[B + 2][H][W] += the rows of x[C][H][W] under t = (x - lo) * scale, 1 <= B <= 62
hipError_t launch_pixel_hist(const float* x, int64_t C, int H, int W, int B, const float* lo, const float* scale, unsigned long long* counts,
                             hipStream_t st);
// chain-group moments (lmc_group_moments.hip): A[G][H][W] += sum x, B[G][H][W] += sum x^2 over the chains of every group of x[C][H][W], the group of
// chain c = (chain_offset + c) mod G; float64, one owner per (group, pixel) and launch, no atomics
hipError_t launch_group_moments(const float* x, int64_t C, int64_t chain_offset, int H, int W, int G, double* A, double* B, hipStream_t st);
// covariance sketch (lmc_cov_sketch.hip): with d_c = x_c - m and t_c[j] = <P_j, d_c>, Y[k][H][W] += sum_c t_c[j] d_c, s[k] += sum_c t_c[j],
// Q[k][k] += sum_c t_c[j] t_c[l]; float64 accumulators, fp32-input MFMA passes, one owner per element and launch, no atomics.  m may be NULL (0);
// ws: cov_sketch_workspace_bytes(C, H, W, k) bytes, 16-byte aligned (0 bytes = bad arguments)
size_t cov_sketch_workspace_bytes(int64_t C, int H, int W, int k);
hipError_t launch_cov_sketch(const float* x, int64_t C, int H, int W, int k, const float* P, const float* m, double* Y, double* s, double* Q, void* ws,
                             hipStream_t st);
hipError_t launch_energies(const float* x, int64_t n_img, const EnergyArgs& E, double* f_out, double* g_out,
                           hipStream_t st);
// ADDS the value of the data term `term` (DataTerm: kTermPois, kTermWl2, kTermHub) to f_out (zeroed by launch_energies): E.data_kind = the operator's kind
// (identity, blur; for Poisson the mask too), E.y = [2][H][W]: counts and background, observation and weights, observation and thresholds
hipError_t launch_energy_term(int term, const float* x, int64_t n_img, const EnergyArgs& E, double* f_out, hipStream_t st);
// pieces of the exact early-exit path of the TV prox (lmc_problem.tv_rtol > 0)
hipError_t launch_tv_objective(const float* x, const float* sol, int64_t n, int H, int W, float gam, const int* flag, double* obj, hipStream_t st);
hipError_t launch_tv_rtol_decide(int64_t n, double* prev, double* cur, int* flag, int pass, double rtol, int* n_active, hipStream_t st);
hipError_t launch_tv_rtol_select(const float* tmp, float* sol, const int* flag, int pass, int64_t n, size_t img, hipStream_t st);
// 1-D TV over the flattened image (inner prox of the anisotropic ME-TV term, algs.py:170): one dual iteration / the primal iterate / its objective
hipError_t launch_tv1d_sol(const float* x, const float* rr, float* out, int64_t n, size_t N, float gam, const int* flag, hipStream_t st);
hipError_t launch_tv1d_iter(const float* x, const float* rr_in, float* p, float* rr_out, int64_t n, size_t N, float gam, float cstep, float beta, const int* flag,
                            hipStream_t st);
hipError_t launch_tv1d_objective(const float* x, const float* sol, int64_t n, size_t N, float gam, const int* flag, double* obj, hipStream_t st);
// the early exit without leaving the device (speculate / verify / re-run; lmc_ops.hip, lmc_tv_exit.hip: tv_prox_rt)
hipError_t launch_tv_rt_begin(int64_t n, const int* pred, int* kc, int* start, double* obj, int stride, int niter, hipStream_t st);
hipError_t launch_tv_rt_decide(int64_t n, int* kc, int* start, int* pred, double* obj, int stride, int niter, double rtol, int round,
                               unsigned long long* reruns, hipStream_t st);
int hbm_copy_probe_shapes();
hipError_t launch_hbm_copy_probe(const float* x, float* y, size_t n_floats, int shape, hipStream_t st);
hipError_t launch_noise(float* out, int C, int H, int W, uint32_t key0, uint32_t key1, uint32_t iteration,
                        uint32_t chain_offset, hipStream_t st);

}  // namespace lmc

namespace lmc {
// HBM-bound tiled kernel for closed-form priors (lmc_step_point.hip)
bool point_supported(const StepArgs& a);
hipError_t launch_step_point(StepArgs a, hipStream_t st);
// register-block kernel for stencil-free data terms and block-local proxes, Haar-l1 included (lmc_step_block.hip)
bool block_supported(const StepArgs& a);
bool block_pair_supported(const StepArgs& a);      // StepArgs::fused_iters = 2
hipError_t launch_step_block(const StepArgs& a, hipStream_t st);
// barrier-free row streaming for a separable blur + closed-form prior (lmc_step_rows.hip)
bool rows_supported(const StepArgs& a);
hipError_t launch_step_rows(StepArgs a, hipStream_t st);
// two MYULA iterations per launch (lmc_step_rows_pair.hip): x_out <- x_{k+2}, x_mid (may be NULL) <- x_{k+1}; three distinct arrays
bool rows_pair_supported(const StepArgs& a);
hipError_t launch_step_rows_pair(StepArgs a, float* x_mid, hipStream_t st);
// taps re-centred for the full-width kernels: returns KT (5 or 7) and fills uc / vc, or 0 (lmc_step_rows.hip)
int centred_blur_taps(const StepArgs& a, float* uc, float* vc);
int centred_blur_taps(const BlurTaps& T, float* uc, float* vc);
// TV stages spread over the waves of a workgroup, one wave = full image width (lmc_step_pipe.hip)
bool pipe_supported(const StepArgs& a);                  // one launch covers it (10 dual iterations)
int pipe_links(const StepArgs& a);                       // launches needed (20 .. 60 iterations: chained through HBM state), 0 = not covered
hipError_t launch_step_pipe(StepArgs a, hipStream_t st, float* state0 = nullptr, float* state1 = nullptr, int teams = 0);   // teams: 0 auto, 1 one-team, 2 two-team
bool pipe_teams_covered(const StepArgs& a, int KT);
// warm-started TV prox: a.tv_in / a.tv_out = [C][2][H][W] projected dual of the previous / this MYULA iteration
bool pipe_warm_supported(const StepArgs& a);
hipError_t launch_step_pipe_warm(StepArgs a, hipStream_t st);
// per-chain early exit of the TV prox (lmc_step_pipe_rt.hip): a.tv.niter in 1 .. 60 dual updates at most, a.rt_kc / rt_obj / rt_stride set by the
// caller; more than 10: a chain of links through state0 / state1 ([C][4][H][W]), pure prox only (no data term, no noise)
bool pipe_rt_supported(const StepArgs& a);
hipError_t launch_step_pipe_rt(StepArgs a, hipStream_t st, float* state0 = nullptr, float* state1 = nullptr);
// split streaming variant: the same pipeline over two wave groups (lmc_step_split.hip)
bool split_supported(const StepArgs& a);
hipError_t launch_step_split(StepArgs a, hipStream_t st);
}  // namespace lmc

namespace lmc {
// ULPDA building blocks (lmc_ulpda.hip)
hipError_t ulpda_dual_update(const float* xhat, float* y, int64_t C, int H, int W, float mu, float radius, int iso, hipStream_t st);
hipError_t ulpda_rhs(const float* x, const float* y, const float* z, const float* htb, float* rhs, int64_t C, int H, int W,
                     float tau, float ts, hipStream_t st);
hipError_t ulpda_me_rhs(const float* v, const float* extra, const float* htb, float* rhs, int64_t C, int H, int W, float coef,
                        float ts, hipStream_t st);
hipError_t ulpda_ncvx_rhs(const float* v, const float* htb, float* rhs, int64_t C, int H, int W, float coef, float gamma, float ts,
                          hipStream_t st);
hipError_t ulpda_pointwise_prox(const float* v, float* u, const float* b, const float* m, int64_t C, int H, int W, float ts,
                                int kind, hipStream_t st);
hipError_t ulpda_finish_philox(float* x, float* xhat, const float* u, int64_t C, int H, int W, float s, float theta, uint32_t key0,
                               uint32_t key1, uint32_t iteration, uint32_t chain_offset, hipStream_t st);
hipError_t ulpda_finish(float* x, float* xhat, const float* u, const float* xi, int64_t C, int H, int W, float s, float theta,
                        hipStream_t st);
hipError_t cg_dot(const float* p, const float* q, int64_t C, size_t img, double* pq, const int* done, hipStream_t st);
hipError_t cg_init(const float* rhs, const float* q, float* r, float* p, int64_t C, size_t img, double* rs, double* b2, hipStream_t st);
hipError_t cg_update(float* u, float* r, const float* p, const float* q, int64_t C, size_t img, const double* rs, const double* pq,
                     double* rs_new, const int* done, hipStream_t st);
hipError_t cg_dir(float* p, const float* r, int64_t C, size_t img, double* rs, const double* rs_new, const int* done, hipStream_t st);
hipError_t cheb_count(int64_t C, const double* stat, double inv_alpha2, double tol, double inv_log_inv_c, int kmax, int* count,
                      hipStream_t st);
hipError_t cg_check(int64_t C, const double* rsv, const double* b2, double tol2, int* done, hipStream_t st);

// Two Chebyshev iterations per launch (lmc_cheb_pair.hip):  f1 = u_{k+1} = a0 cur - t0 sigma H^T H cur + b0 rhs + s0 prv,
// f2 (or f2_last) = u_{k+2} = a1 f1 - t1 sigma H^T H f1 + b1 rhs + s1 cur.  tg = t sigma_f c_u c_v (the launcher fills cbox and folds it in).
// The launch returns at once when *run_count <= run_index; it writes u_{k+2} to f2_last instead of f2 when force_last or *run_count <= last_index
// (no later pair of the solve will run).  cur, prv, rhs, f1, f2, f2_last: [C][H][W]; f1, f2, f2_last distinct from the inputs.
struct ChebPairArgs {
  int H, W, C;
  float cbox;
  const float* cur;
  const float* prv;
  const float* rhs;
  float* f1;
  float* f2;
  float* f2_last;
  float a0, tg0, b0, s0, a1, tg1, b1, s1;
  const int* run_count;
  int run_index, last_index, force_last;
  double* dot_out;      // non-NULL: dot_out[2c] += sum (f1 - cur)^2, dot_out[2c+1] += sum rhs^2 (the statistics the adaptive iteration count is made from)
};
bool cheb_pair_supported(int H, int W, const BlurTaps& taps);
bool cheb_pair_pays(int64_t C, int H);
hipError_t launch_cheb_pair(ChebPairArgs a, const BlurTaps& taps, hipStream_t st);
}  // namespace lmc

namespace lmc {
// Metropolis adjustment glue (lmc_mala.hip)
hipError_t mala_propose(const float* mx, const float* xi, float* xp, int64_t C, size_t img, float s, double* d1, hipStream_t st);
hipError_t mala_propose_philox(const float* mx, float* xp, int64_t C, int H, int W, float s, uint32_t key0, uint32_t key1,
                               uint32_t iteration, uint32_t chain_offset, double* d1, hipStream_t st);
hipError_t mala_accept(int C, double* U, const double* fp, const double* gp, float epsg, const double* d1, const double* d2, float tau,
                       uint32_t key0, uint32_t key1, uint32_t iteration, uint32_t chain_offset, int* flag,
                       unsigned long long* nacc, double* log_alpha, hipStream_t st);
hipError_t mala_select(const int* flag, float* x, float* mx, const float* xp, const float* mxp, int64_t C, size_t img, int when,
                       hipStream_t st);
}  // namespace lmc

namespace lmc {
// SAPG estimation of the prior weight (lmc_sapg.hip).  stat[i] = g(x_i) with weight 1 for LMC_PRIOR_L2 / L1 / TV_ISO / TV_ANISO / HAAR_L1 (other
// kinds: hipErrorInvalidValue), every image summed in a fixed order.  An image is read by prior_stat_segments(n_img, H) workgroups; when that is
// more than one, `part` holds n_img * segments doubles for their partial sums (else it may be NULL).
struct SapgParams;
int prior_stat_segments(int64_t n_img, int H);
hipError_t launch_prior_stat(const float* x, int64_t n_img, int H, int W, int prior_kind, double* stat, double* part, hipStream_t st);
// one workgroup: gbar = mean of stat[C] (fixed order), theta_trace[n + 1] = the update of `theta`, gbar_trace[n] = gbar, host2[0 .. 1] = both
hipError_t launch_sapg_update(const double* stat, int C, const SapgParams& P, long long n, double theta, double* theta_trace, double* gbar_trace,
                              double* host2, hipStream_t st);
}  // namespace lmc

namespace lmc {
// Large point-spread functions (lmc_psf.hip, lmc_psf_kernel.h): the operator of LMC_DATA_PSF and lmc_psf_apply, kernels up to kPsfMax x kPsfMax.
constexpr int kPsfMax = LMC_MAX_PSF;
constexpr int kPsfKP = 40;                                   // tap rows of the device table: kPsfMax padded to whole blocks of 8
constexpr int kPsfTabFloats = 2 * kPsfMax * kPsfKP;          // the table of one direction (general form, or the two factors in its head); H then H^T
// what a launch does with u = H x or H^T x
enum PsfEpi {
  kPsfRaw = 0,      // out = u
  kPsfRhoL2,        // out = u - y
  kPsfRhoWl2,       // out = w (u - y),            y = [2][H][W]: observation, weights
  kPsfRhoPois,      // out = pois_rho(u, y, beta), y = [2][H][W]: counts, background
  kPsfSub,          // out -= coef u
  kPsfOverwrite,    // out = a xin - coef u
  kPsfEnL2,         // part[image][tile] = sum 1/2 (u - y)^2        (no store of u)
  kPsfEnWl2,        // part[image][tile] = sum 1/2 w (u - y)^2
  kPsfEnPois,       // part[image][tile] = sum pois_phi(u, y, beta)
  // (appended: the values above are template arguments of kernels that keep their names)
  kPsfRhoHub,       // out = clamp(u - y, -delta, delta),  y = [2][H][W]: observation, thresholds (the Huber term)
  kPsfEnHub         // part[image][tile] = sum hub_h(u - y, delta)
};
// the residual and the energy epilogue of a data term, indexed by DataTerm (lmc_common.h)
struct PsfTermEpi { PsfEpi rho, energy; };
constexpr PsfTermEpi kPsfTermEpi[kNumTerms] = {{kPsfRhoL2, kPsfEnL2}, {kPsfRhoPois, kPsfEnPois}, {kPsfRhoWl2, kPsfEnWl2}, {kPsfRhoHub, kPsfEnHub}};
// Host description of a validated PSF and the device table made from it.  tab (host) / tab_dev: [2][kPsfMax * kPsfKP] floats, direction 0 = H (taps
// flipped, origin mirrored), 1 = H^T, each in the correlation form of the kernel: general g[b * kPsfKP + a], separable gu[kPsfKP] then gv[kPsfKP].
struct PsfOp {
  int on = 0;                 // the problem's operator is a PSF
  int kh = 0, kw = 0, oy = 0, ox = 0;
  int separable = 0;          // the two-pass form
  float tab[kPsfTabFloats] = {};
  const float* tab_dev = nullptr;      // set by whoever owns the device copy (a sampler handle, the stateless scratch)
  float* resid = nullptr;              // [C][H][W] residual buffer of the step, same owner
};
// 1 / 0: h is an outer product by the criterion of lmc_psf_separable (u, v may be NULL)
int psf_separable(const float* h, int kh, int kw, float* u, float* v);
// fills kh .. separable and tab from validated geometry; mode: lmc_problem.psf_separable (0 auto, 1 require, 2 forbid).  false: mode 1 on a kernel that
// fails the criterion
bool psf_prepare(PsfOp& P, const float* h, int kh, int kw, int oy, int ox, int mode);
// epi: PsfEpi, store forms only (kPsfRaw .. kPsfOverwrite, kPsfRhoHub).  out = epilogue(H x or H^T x); xin: kPsfOverwrite; y: the rho forms
hipError_t launch_psf(const PsfOp& P, int adjoint, int epi, const float* x, float* out, const float* xin, const float* y, int64_t n_img, int H, int W,
                      float a, float coef, hipStream_t st);
// doubles `part` must hold for launch_psf_energy
size_t psf_energy_partials(int64_t n_img, int H, int W);
// f_out[c] += the data term's value at x_c (term: DataTerm), float64 by partial sums in a fixed order
hipError_t launch_psf_energy(const PsfOp& P, int term, const float* x, const float* y, int64_t n_img, int H, int W, float sigma_f, double* part,
                             double* f_out, hipStream_t st);
}  // namespace lmc

namespace lmc {
// SK-ROCK stage 1 (lmc_skrock.hip): out = x + coef * Z, Z the Philox / Box-Muller field of `iteration` that the step kernels and launch_noise draw
// (same device functions, same counter layout: bit for bit that field), or the caller's field xi.  x, out (and xi): [C][H][W] / n floats, distinct.
hipError_t launch_skrock_perturb_philox(const float* x, float* out, int64_t C, int H, int W, float coef, uint32_t key0, uint32_t key1,
                                        uint32_t iteration, uint32_t chain_offset, hipStream_t st);
hipError_t launch_skrock_perturb(const float* x, const float* xi, float* out, size_t n, float coef, hipStream_t st);
}  // namespace lmc

namespace lmc {
// Daubechies wavelet-l1 prior (lmc_wavelet.hip): the periodic multi-level transform of db1 .. db4, its prox and its value.
constexpr int kWaveletMaxP = 4;
// The prior of a validated problem and the device workspace of whoever owns it (a sampler handle, the stateless scratch): ws holds
// wavelet_ws_floats(n, H, W) floats (the thresholded pyramid and the LL ping-pong: 1.25 states), part n * wavelet_partials(H, W, levels) doubles.
struct WaveletOp {
  int on = 0;
  int p = 0, levels = 0;
  float* ws = nullptr;
  double* part = nullptr;
};
bool wavelet_shape_ok(int H, int W, int p, int levels);       // the preconditions of include/lmc_atomi.h
int wavelet_filter(int p, double* h);                         // taps in float64 into h[2p], returns 2p (0: bad p)
size_t wavelet_ll_floats(int64_t n_img, int H, int W);        // the approximations of level 1
size_t wavelet_ws_floats(int64_t n_img, int H, int W);
int wavelet_partials(int H, int W, int levels);
// out = W^T soft(W x, thr); x != out; ws: wavelet_ws_floats
hipError_t launch_wavelet_prox(const float* x, float* out, int64_t n_img, int H, int W, int p, int levels, float thr, float* ws, hipStream_t st);
// val[i] = sigma * sum |details of x_i|; ws: 5/4 wavelet_ll_floats (+ 1), part: n_img * wavelet_partials doubles
hipError_t launch_wavelet_value(const float* x, int64_t n_img, int H, int W, int p, int levels, float sigma, float* ws, double* part, double* val,
                                hipStream_t st);
// out = W x or W^T x (Mallat layout); x != out; ws as for the value
hipError_t launch_wavelet_apply(const float* x, float* out, int64_t n_img, int H, int W, int p, int levels, int inverse_dir, float* ws, hipStream_t st);
}  // namespace lmc

namespace lmc {
// Vectorial TV (lmc_vtv.hip): the prox and the value of LMC_PRIOR_VTV on channel-major multi-channel images, image (ch, n) at x + ch * cs + n * H * W.
constexpr int kVtvMaxChannels = LMC_MAX_CHANNELS;
// The launch plan of a prox of niter dual iterations on nch channels: a workgroup owns a PH x PW patch = a TH x TW tile plus a halo of HL pixels, which
// covers the `iters` dual iterations of one launch; n_launches launches are chained through the dual state.  Host only.
struct VtvPlan {
  int PH, PW, HL, TH, TW;
  int iters, n_launches;
  size_t lds_bytes;           // dynamic LDS of one workgroup
};
bool vtv_plan(int nch, int niter, VtvPlan& out);       // false: nch outside 1 .. kVtvMaxChannels or niter outside 1 .. kMaxTvIters
// floats each of the two state buffers of a chained prox holds ([n_img][nch][4][H][W]); 0 when one launch covers niter
size_t vtv_state_floats(int64_t n_img, int nch, int H, int W, int niter);
// out = prox of gamma * VTV at x (gamma = t sigma > 0), niter dual iterations of step `step` / gamma with the momentum table betas[niter] (host); box != 0:
// the constrained form on [box_lo, box_hi].  x != out, both with channel stride cs.  state0 / state1: vtv_state_floats each (may be NULL when that is 0).
hipError_t launch_vtv_prox(const float* x, float* out, int64_t n_img, int nch, int64_t cs, int H, int W, float gamma, float step, const float* betas, int niter,
                           int box, float box_lo, float box_hi, float* state0, float* state1, hipStream_t st);
// doubles `part` must hold for launch_vtv_value
size_t vtv_value_partials(int64_t n_img, int H, int W);
// val[n] = scale * VTV(x_n), float64 by partial sums in a fixed order
hipError_t launch_vtv_value(const float* x, int64_t n_img, int nch, int64_t cs, int H, int W, double scale, double* part, double* val, hipStream_t st);
}  // namespace lmc

namespace lmc {
// Second-order TGV (lmc_tgv.hip): the prox of LMC_PRIOR_TGV on single-plane images [n][H][W] by Chambolle-Pock primal-dual iterations.
constexpr int kMaxTgvIters = LMC_MAX_TGV_ITERS;
#ifndef LMC_TGV_LAUNCH_ITERS
#define LMC_TGV_LAUNCH_ITERS 6           // chosen by measurement (DESIGN 3.0p "TGV prior"); -DLMC_TGV_LAUNCH_ITERS=n on lmc_tgv.hip and lmc_capi.hip measures another
#endif
constexpr int kTgvLaunchIters = LMC_TGV_LAUNCH_ITERS;      // iterations one launch holds (its halo): at 6 a 52 x 52 tile of the 64 x 64 patch, 1.51 pixel updates per pixel
constexpr float kTgvStep = 0.28867513f;  // 1 / sqrt(12): ||K||^2 < 12 for K = [[grad, -I], [0, E]]
// The launch plan of a prox of niter iterations: a workgroup owns a PH x PW patch = a TH x TW tile plus a halo of HL pixels, which covers the `iters`
// iterations of one launch; n_launches launches are chained through the 11-plane state.  Host only.
struct TgvPlan {
  int PH, PW, HL, TH, TW;
  int iters, n_launches;
  size_t lds_bytes;           // dynamic LDS of one workgroup
};
bool tgv_plan(int niter, TgvPlan& out);       // false: niter outside 1 .. kMaxTgvIters
// floats each of the two state buffers of a chained prox holds ([n_img][11][H][W]); 0 when one launch covers niter
size_t tgv_state_floats(int64_t n_img, int H, int W, int niter);
// out = prox_{t g}(x) with lam1 = t sigma > 0 by niter iterations of step `step` for both sides; w_out: NULL or [n][2][H][W], the auxiliary field;
// box != 0: the primal iterate of every iteration clipped to [box_lo, box_hi].  x != out.  state0 / state1: tgv_state_floats each (may be NULL when 0).
hipError_t launch_tgv_prox(const float* x, float* out, float* w_out, int64_t n_img, int H, int W, float lam1, float alpha0, float step, int niter, int box,
                           float box_lo, float box_hi, float* state0, float* state1, hipStream_t st);
}  // namespace lmc

namespace lmc {
// The spectral data term (lmc_fft.hip, lmc_fft_kernel.h): the batched 2-D real FFT in LDS of LMC_DATA_SPECTRAL, lmc_rfft2 / lmc_irfft2 and
// lmc_spectral_filter; power-of-two sides kFftMin .. kFftMax, the half plane of W / 2 + 1 columns, norm = "ortho".
constexpr int kFftMin = 8, kFftMax = 1024;
constexpr int kFftTw = kFftMax;           // entries of the twiddle table: exp(-2 pi i m / kFftTw)
constexpr int kFftThreads = 512;          // eight waves share the two LDS buffers of a workgroup: two workgroups per CU, four waves per SIMD
constexpr int kFftElems = 4096;           // complex values of one of a workgroup's two LDS buffers: kFftElems / N lines of length N
constexpr int kFftPlanes = 11;            // planes [H][Wh] of the descriptor at lmc_problem.y_dev
// what fft_rows_inv_kernel does with the real part v of the inverted row
enum FftEpi {
  kFftStore = 0,    // out = v
  kFftSub,          // out -= coef v
  kFftOverwrite     // out = a x - coef v
};
// what fft_cols_spectral_kernel does between (or in place of) its two column transforms
enum FftMode {
  kFftColFwd = 0,   // forward only
  kFftColInv,       // inverse only
  kFftGrad,         // A xh - B
  kFftProx,         // (vh + ts B) / (1 + ts A)
  kFftMul,          // M xh
  kFftValue         // part[image][strip] = sum |G xh - b|^2 + |conj(G_-k) xh - conj(b_-k)|^2
};
// The operator of a validated problem and the device buffers of whoever owns them (a sampler handle, the stateless scratch): tw the twiddle table
// (fft_twiddles), spec [n][H][W / 2 + 1] complex, part fft_value_partials doubles.
struct FftOp {
  int on = 0;
  const float* tab = nullptr;       // lmc_problem.y_dev: [kFftPlanes][H][Wh]
  const float2* tw = nullptr;
  float2* spec = nullptr;
  double* part = nullptr;
};
bool fft_shape_ok(int H, int W);
void fft_twiddles(float* tw_host /* [2 * kFftTw] */);     // float64 sine and cosine, rounded once
size_t fft_spec_floats(int64_t n_img, int H, int W);
size_t fft_value_partials(int64_t n_img, int H, int W);
// host: the descriptor planes from G and b ([H][W] complex, interleaved float64), folded in float64
void fft_tables(const double* G, const double* b, int H, int W, float* out);
hipError_t launch_fft_rows_fwd(const float* x, float2* spec, const float2* tw, int64_t n_img, int H, int W, hipStream_t st);
// mode: FftMode but kFftValue; tab: the planes the functor reads
hipError_t launch_fft_cols(int mode, float2* spec, const float* tab, const float2* tw, int64_t n_img, int H, int W, float ts, hipStream_t st);
// The column pass of the split Gibbs sampler's x-draw (sgs_cols_gibbs_kernel, lmc_sgs_kernel.h), in place in zspec (the row transform of z): the column transform of nspec (the row
// transform of a white field; NULL: no noise, the conditional mean) is kept in registers scaled by sqrt(q), then zspec is transformed, the functor
// (zh rinv + sf B + sqrt(q) nh) / q with q = sf A + rinv is applied and the result transformed back.  tab: planes A, Re B, Im B.  nspec is only read.
hipError_t launch_fft_gibbs(float2* zspec, const float2* nspec, const float* tab, const float2* tw, int64_t n_img, int H, int W, float rinv, float sf,
                            hipStream_t st);
// epi: FftEpi; xin: kFftOverwrite
hipError_t launch_fft_rows_inv(int epi, const float2* spec, float* out, const float* xin, const float2* tw, int64_t n_img, int H, int W, float a, float coef,
                               hipStream_t st);
// f_out[c] += sigma_f / 2 * the half-plane sum at x_c, float64 by partial sums in a fixed order
hipError_t launch_fft_value(const FftOp& F, const float* x, int64_t n_img, int H, int W, float sigma_f, double* f_out, hipStream_t st);
}  // namespace lmc

namespace lmc {
// The multi-coil SENSE data term (lmc_sense.hip, lmc_sense_kernel.h): the operator of LMC_DATA_SENSE and lmc_sense_apply; lmc_atomi.h holds its definition.
// The complex full plane of W columns through the transforms, sides and twiddle table of the spectral term above, one coil at a time.
constexpr int kSenseMaxCoils = LMC_MAX_COILS;
// what sense_rows_inv_kernel does with v = Re[conj(S_c) .] of the inverted row
enum SenseEpi {
  kSenseStore = 0,  // out = v      (coil 0)
  kSenseAdd         // out += v     (the coils after it)
};
// what sense_cols_kernel does around its column transforms
enum SenseMode {
  kSenseGrad = 0,   // forward, M (M v - b_c), inverse
  kSenseValue,      // forward, part[image][strip] = sum |M v - b_c|^2
  kSenseFwd,        // forward, M v
  kSenseAdj         // M v, inverse
};
// The operator of a validated problem and the device buffers of whoever owns them (a sampler handle, the stateless scratch): desc the descriptor at
// lmc_problem.y_dev ([1 + 4 n_coils][H][W]: M, then Re / Im of every S_c, then Re / Im of every b_c), tw the twiddle table (fft_twiddles), spec
// [n][H][W] complex, g [n][H][W] the gradient image of a step, part sense_value_partials doubles.
struct SenseOp {
  int on = 0;
  int n_coils = 0;
  const float* desc = nullptr;
  const float2* tw = nullptr;
  float2* spec = nullptr;
  float* g = nullptr;
  double* part = nullptr;
};
size_t sense_spec_floats(int64_t n_img, int H, int W);
size_t sense_value_partials(int64_t n_img, int H, int W);
int sense_strips(int H, int W);
// the kernels' launchers (lmc_fft.hip).  s: Re S_c, Im S_c one plane after it; b likewise; strides in complex values between the images
hipError_t launch_sense_rows_fwd(const float* x, const float* s, float2* spec, int64_t spec_stride, const float2* tw, int64_t n_img, int H, int W, hipStream_t st);
// mode: SenseMode; src == spec where the pass runs in place; b: kSenseGrad / kSenseValue; part: kSenseValue
hipError_t launch_sense_cols(int mode, const float2* src, int64_t src_stride, float2* spec, int64_t spec_stride, const float* m, const float* b, double* part,
                             const float2* tw, int64_t n_img, int H, int W, hipStream_t st);
// epi: SenseEpi; spec dense
hipError_t launch_sense_rows_inv(int epi, const float2* spec, const float* s, float* out, const float2* tw, int64_t n_img, int H, int W, hipStream_t st);
// f_out[c] += scale * the sum of part[c][.] in strip order
hipError_t launch_sense_value_finish(const double* part, int64_t n_img, int strips, double scale, double* f_out, hipStream_t st);
// alone: out = a x - coef g; else out -= coef g; n floats
hipError_t launch_sense_axpy(bool alone, const float* g, const float* x, float* out, size_t n, float a, float coef, hipStream_t st);
// the coil loops (lmc_sense.hip), coils in the order c = 0, 1, ...
// S.g = sum_c Re[conj(S_c) F^H(M (M F(S_c x) - b_c))] at the n_img images x
hipError_t launch_sense_gradient(const SenseOp& S, const float* x, int64_t n_img, int H, int W, hipStream_t st);
// f_out[i] += sigma_f / 2 sum_c sum_k |M F(S_c x_i) - b_c|^2, float64 by partial sums in a fixed order
hipError_t launch_sense_value(const SenseOp& S, const float* x, int64_t n_img, int H, int W, float sigma_f, double* f_out, hipStream_t st);
// adjoint == 0: in real [n][H][W] -> out complex [n][n_coils][H][W], M F(S_c x); else that shape -> real [n][H][W], sum_c Re[conj(S_c) F^H(M k_c)].  Reads
// desc, tw and spec of S (the data planes of desc are not read)
hipError_t launch_sense_apply(const SenseOp& S, const float* in, float* out, int64_t n_img, int H, int W, int adjoint, hipStream_t st);
// host: max M^2 * max_p sum_c |S_c(p)|^2 from the descriptor, in float64
double sense_lipschitz(const float* desc_host, int H, int W, int n_coils);
}  // namespace lmc

namespace lmc {
// The parallel-beam Radon operator (lmc_radon.hip, lmc_radon_kernel.h): the operator of LMC_DATA_RADON .. LMC_DATA_HUBER_RADON and lmc_radon_apply;
// lmc_atomi.h holds its definition.  Sinograms are [n_img][n_angles][n_det] floats.
constexpr int kRadonMaxAngles = LMC_MAX_RADON_ANGLES;
constexpr int kRadonMaxDet = LMC_MAX_RADON_DET;
constexpr int kRadonMaxSide = 1 << 20;        // sides up to here: the forward kernel's column estimate stays within its margin (lmc_radon_kernel.h)
// what a launch does with u = A x (forward: a sinogram) or A^T r (adjoint: an image)
enum RadonEpi {
  kRadonRaw = 0,      // out = u
  kRadonRhoL2,        // out = u - y                                    (forward; y = [n_angles][n_det])
  kRadonRhoPois,      // out = pois_rho(u, y, beta)                     (forward; y = [2][n_angles][n_det]: counts, background)
  kRadonRhoWl2,       // out = w (u - y)                                (forward; observation, weights)
  kRadonRhoHub,       // out = clamp(u - y, -delta, delta)              (forward; observation, thresholds)
  kRadonEnL2,         // part[image][block] = sum 1/2 (u - y)^2         (forward; no store of u)
  kRadonEnPois,       // part[image][block] = sum pois_phi(u, y, beta)
  kRadonEnWl2,        // part[image][block] = sum 1/2 w (u - y)^2
  kRadonEnHub,        // part[image][block] = sum hub_h(u - y, delta)
  kRadonSub,          // out -= coef u                                  (adjoint)
  kRadonOverwrite     // out = a xin - coef u                           (adjoint)
};
// the residual and the energy epilogue of a data term, indexed by DataTerm (lmc_common.h)
struct RadonTermEpi { RadonEpi rho, energy; };
constexpr RadonTermEpi kRadonTermEpi[kNumTerms] = {{kRadonRhoL2, kRadonEnL2}, {kRadonRhoPois, kRadonEnPois}, {kRadonRhoWl2, kRadonEnWl2}, {kRadonRhoHub, kRadonEnHub}};
// Host description of a validated operator and the device buffers of whoever owns them (a sampler handle, the stateless scratch).  The forward kernel
// walks image rows for an angle with |cos| >= |sin| and image columns for the others; order lists the angles of the first kind, then the rest.
struct RadonOp {
  int on = 0;                 // the problem's operator is the Radon operator
  int n_angles = 0, n_det = 0;
  int n_row = 0;              // angles with |cos| >= |sin|: order[0 .. n_row)
  float angles[kRadonMaxAngles] = {};
  int order[kRadonMaxAngles] = {};
  const float* tab_dev = nullptr;      // radon_table_floats: ax[n_angles][W], by[n_angles][H], the reciprocal slopes [n_angles], order [n_angles] (ints)
  float* resid = nullptr;              // [n][n_angles][n_det] residual buffer of the step
};
// fills n_angles .. order from validated arguments (finite angles, 1 <= n_angles <= kRadonMaxAngles, 1 <= n_det <= kRadonMaxDet)
void radon_prepare(RadonOp& R, const float* angles, int n_angles, int n_det);
size_t radon_table_floats(int n_angles, int H, int W);
// host: the device table of R on H x W images (float64 products, rounded once)
void radon_tables(const RadonOp& R, int H, int W, float* out);
// epi: kRadonRaw or a rho form; out = epilogue(A x), [n_img][n_angles][n_det]
hipError_t launch_radon_forward(const RadonOp& R, int epi, const float* x, float* out, const float* y, int64_t n_img, int H, int W, hipStream_t st);
// epi: kRadonRaw, kRadonSub, kRadonOverwrite; out = epilogue(A^T r), [n_img][H][W]; xin: kRadonOverwrite
hipError_t launch_radon_adjoint(const RadonOp& R, int epi, const float* r, float* out, const float* xin, int64_t n_img, int H, int W, float a, float coef,
                                hipStream_t st);
// doubles `part` must hold for launch_radon_energy
size_t radon_energy_partials(const RadonOp& R, int64_t n_img);
// f_out[c] += sigma_f * the data term's value at x_c (term: DataTerm), float64 by partial sums in a fixed order
hipError_t launch_radon_energy(const RadonOp& R, int term, const float* x, const float* y, int64_t n_img, int H, int W, float sigma_f, double* part,
                               double* f_out, hipStream_t st);
}  // namespace lmc
