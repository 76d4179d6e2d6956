// Internals of the C-ABI host code, shared by its translation units (not installed):
//   lmc_capi.hip        the stateless extern "C" entry points, the last error, the stateless scratch
//   lmc_problem.hip     lmc_problem -> Problem, StepArgs of an update, the step-kernel dispatch, the library defaults
//   lmc_solve.hip       the implicit step (I + ts H^T H) u = rhs: Chebyshev, CG
//   lmc_tv_exit.hip     the early exits of the TV prox, the ME-TV inner prox and envelope
//   lmc_sampler.hip     the MYULA, MYMALA, SK-ROCK and ULPDA samplers: create / destroy, state, the step loops
//   lmc_accum.hip       the accumulators over the kept samples (lmc_accum.h): their reductions and their set / get / reset entry points
//   lmc_rccl.hip        the dlopen'd RCCL and the all-reduces of the accumulators
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "lmc_accum.h"
#include "lmc_launch.h"

namespace lmc::host {

// Uniform boxes (all the reference's blurs): the KT centred taps t are one constant on one window [lo, hi] and zero elsewhere.  The step kernels that
// have a shared-sum form for such taps (rows: lmc_step_rows.hip, pipe: lmc_step_pipe.hip) take it when rows and columns have the same window; other taps
// take the general form.
inline bool uniform_window(const float* t, int KT, int& lo, int& hi) {
  lo = -1; hi = -1;
  for (int i = 0; i < KT; ++i) if (t[i] != 0.f) { if (lo < 0) lo = i; hi = i; }
  if (lo < 0) return false;
  for (int i = lo; i <= hi; ++i) if (std::fabs(t[i] - t[lo]) > 1e-6f * std::fabs(t[lo])) return false;
  return true;
}

// Records the message lmc_last_error returns and passes `code` on.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(LMC_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Closed-form proxes: the parameters that are weights, scales or bounds must be >= 0 (a negative one has no prox, and the closed forms take square roots of
// it); 0 is allowed (the prox of the zero function is the identity).  NaN fails too.  Bit i of the table = parameter i is such a parameter.
inline bool eprox_params_ok(int kind, float p0, float p1) {
  static const unsigned char nonneg[] = {1, 1, 1, 1, 1, 1, 1, 3, 1, 1, 3, 1, 1, 0, 0};
  return (!(nonneg[kind] & 1) || p0 >= 0.f) && (!(nonneg[kind] & 2) || p1 >= 0.f);
}

// Validated, self-contained copy of an lmc_problem.
struct Problem {
  int H = 0, W = 0;
  int data_kind = 0;        // the operator's kind, LMC_DATA_NONE .. LMC_DATA_MASK (a Poisson term: with pois = 1)
  int wl2 = 0;              // LMC_DATA_WL2_*: per-pixel weights on the Gaussian term of that operator; y is [2][H][W], observation then weights
  int pois = 0;             // LMC_DATA_POISSON_*: the Poisson likelihood on that operator; y is [2][H][W], counts then background
  float sigma_f = 0.f;
  const float* y = nullptr;
  const float* mask = nullptr;
  lmc::BlurTaps taps{};
  lmc::PsfOp psf;           // LMC_DATA_PSF / POISSON_PSF / WL2_PSF: data_kind = LMC_DATA_PSF (with pois / wl2), the operator and its device table
  lmc::FftOp fft;           // LMC_DATA_SPECTRAL: the planes at y_dev and the device buffers of whoever owns them
  int prior_kind = 0;
  float prior_sigma = 0.f;
  lmc::WaveletOp wav;       // LMC_PRIOR_WAVELET_L1: p, levels and the workspace of whoever owns it
  int tv_niter = 0;
  float tv_step = 0.125f;
  float betas[lmc::kMaxTvIters] = {};
  int ncvx_kind = 0;
  float ncvx_lambda = 0.f, ncvx_gamma = 1.f;
  int ncvx_niter = 0;
  int ncvx_aniso = 0;       // ME-TV: the 1-D TV of the flattened image (LMC_NCVX_ME_TV_ANISO)
  int tv_warm = 0;
  int tv_warm_asked = 0;    // lmc_problem.tv_warm as given (tv_warm: where the prior has a warm dual)
  int tv_niter_asked = 0;   // lmc_problem.tv_niter as given (tv_niter: after tv_lagged_output)
  float tv_rtol = 0.f;      // > 0: pyproximal.TV's per-image early exit (device path tv_prox_rt, or the pass-by-pass path tv_prox_rtol)
  float ncvx_rtol = 0.f;    // > 0: the same for the inner prox of the ME-TV term (device path only)
  int tv_exit_path = 0;     // 1: always pass by pass
  int iters_per_launch = 0, moments_overlap = 0, moments_bg_wgs = 0;   // launch policy (0 = library decides; fixed at sampler creation)
  int cheb_pair = 1;        // two Chebyshev iterations per launch: 0 never, 1 where they pay, 2 wherever covered
  int eprox_kind = 0, eprox_mask = 0;   // LMC_PRIOR_EPROX: closed form, which parameters scale with the prox parameter
  float eprox_p0 = 0.f, eprox_p1 = 0.f;
  const float* prox_scale = nullptr;   // array-valued epsg: per-chain / per-pixel multiplier of the prox parameter (closed-form priors of MYULA only)
  int64_t prox_scale_cs = 0, prox_scale_ps = 0;
  int box = 0;              // lmc_problem.box_enable: x in [box_lo, box_hi], the prox is that of g + the indicator of the box
  float box_lo = 0.f, box_hi = 0.f;
  int variant = 0;          // 0: the library default (g_variant)
  float implicit_tol = 0.f; // 0: the library default (g_cg_tol); < 0: disabled
};

// Buffers of the device-side early exit of a TV prox (tv_prox_rt): per chain the pass count of the current round (kc; -1 = settled), the pass it left
// in at the previous call (pred: the prediction of the next one), the primal objectives of the iterates [n][stride], and three counters of re-runs.
struct RtState {
  int* kc = nullptr;
  int* start = nullptr;
  int* pred = nullptr;
  double* obj = nullptr;
  unsigned long long* reruns = nullptr;     // [4]: chains that had to run again after rounds 1 .. 4 (the last stays 0 by construction)
  int stride = 0;
  size_t n = 0;
  hipError_t need(size_t n_img, int niter) {
    if (n_img <= n && niter + 1 <= stride) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&kc, sizeof(int) * n_img);
    if (e == hipSuccess) e = hipMalloc(&start, sizeof(int) * n_img);
    if (e == hipSuccess) e = hipMalloc(&pred, sizeof(int) * n_img);
    if (e == hipSuccess) e = hipMalloc(&obj, sizeof(double) * n_img * (size_t)(niter + 1));
    if (e == hipSuccess) e = hipMalloc(&reruns, sizeof(unsigned long long) * 4);
    if (e == hipSuccess) e = hipMemset(pred, 0, sizeof(int) * n_img);           // 0 = no prediction yet: the first call runs every pass
    if (e == hipSuccess) e = hipMemset(reruns, 0, sizeof(unsigned long long) * 4);
    if (e == hipSuccess) { n = n_img; stride = niter + 1; }
    return e;
  }
  void release() {
    if (kc) (void)hipFree(kc);
    if (start) (void)hipFree(start);
    if (pred) (void)hipFree(pred);
    if (obj) (void)hipFree(obj);
    if (reruns) (void)hipFree(reruns);
    kc = start = pred = nullptr; obj = nullptr; reruns = nullptr; n = 0; stride = 0;
  }
};

// Device scratch for the stateless entry points (grown on demand and never freed: it lives for the life of the process; calls are
// serialised by the caller, see lmc_atomi.h).  Samplers own their buffers instead.
struct Scratch {
  float* state[2] = {nullptr, nullptr};   // TV dual state ping-pong, [n][4][H][W] each
  float* extra = nullptr;                 // ME-TV inner prox, [n][H][W]
  float* prox = nullptr;                  // Haar-l1 prox / early-exit TV prox, [n][H][W]
  float* rtmp = nullptr;                  // early-exit TV prox: the iterate of the current pass, [n][H][W]
  double* dbl = nullptr;                  // 2*n doubles
  float* resid = nullptr;                 // large PSF: the residual rho(H x) of a step, [n][H][W]
  float* wav = nullptr;                   // wavelet prior: the thresholded pyramid and the LL ping-pong
  double* wav_part = nullptr;             // wavelet prior: the partial sums of its value
  // large PSF: the device tap table of the stateless calls, the pinned host copy it was uploaded from (compared with the next call's table: equal
  // taps are not uploaded again) and the event behind the last upload (the host copy is not rewritten before that upload has run)
  float* psf_tab = nullptr;
  float* psf_host = nullptr;
  hipEvent_t psf_ev = nullptr;
  bool psf_valid = false;
  // spectral data term: the twiddle table (uploaded once), the spectrum buffer [n][H][Wh] complex, the partial sums of the value
  float* fft_tw = nullptr;
  float* fft_spec = nullptr;
  double* fft_part = nullptr;
  size_t n_fft_spec = 0, n_fft_part = 0;
  size_t n_resid = 0, n_wav = 0, n_wav_part = 0;
  RtState rt_tv, rt_me;                   // device-side early exit of the TV prior's prox / of the ME-TV inner prox
  size_t n_state[2] = {0, 0}, n_extra = 0, n_prox = 0, n_rtmp = 0, n_dbl = 0;   // elements allocated
  // p holds at least n elements afterwards; what it held is not kept when it grows
  template <class T>
  static hipError_t grow(T*& p, size_t& have, size_t n) {
    if (n <= have) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; have = 0;
    hipError_t e = hipMalloc(&p, sizeof(T) * n);
    if (e == hipSuccess) have = n;
    return e;
  }
  hipError_t need_state(size_t n) {
    hipError_t e = grow(state[0], n_state[0], n);
    return e == hipSuccess ? grow(state[1], n_state[1], n) : e;
  }
  hipError_t need_extra(size_t n) { return grow(extra, n_extra, n); }
  hipError_t need_prox(size_t n) { return grow(prox, n_prox, n); }
  hipError_t need_rtmp(size_t n) { return grow(rtmp, n_rtmp, n); }
  hipError_t need_dbl(size_t n) { return grow(dbl, n_dbl, n); }
  hipError_t need_resid(size_t n) { return grow(resid, n_resid, n); }
  hipError_t need_fft(size_t n_spec, size_t n_part) {
    hipError_t e = grow(fft_spec, n_fft_spec, n_spec);
    return e == hipSuccess && n_part ? grow(fft_part, n_fft_part, n_part) : e;
  }
  hipError_t need_wav(size_t n, size_t n_part) {
    hipError_t e = grow(wav, n_wav, n);
    return e == hipSuccess && n_part ? grow(wav_part, n_wav_part, n_part) : e;
  }
  // frees the wavelet workspace (the largest buffer a stateless call takes: 1.25 states); the next call that needs it allocates again
  void release() {
    if (wav) (void)hipFree(wav);
    if (wav_part) (void)hipFree(wav_part);
    wav = nullptr; wav_part = nullptr; n_wav = 0; n_wav_part = 0;
  }
};
// The scratch of the current device: a process may drive several GPUs (one sampler handle each); the stateless entry points run on the current device.
Scratch& scratch_here();

// Makes `dev` the current device for the duration of a call on a handle that lives there, and restores the caller's device.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// batches of side-stream moment reductions one lmc_sampler_step call keeps in flight (the default policies have two at a time; one more
// first waits for the oldest)
constexpr int kSideBatches = 4;

// ---- lmc_problem.hip ----
int fill_taps(lmc::BlurTaps& T, const float* h, int kh, int kw, int oy, int ox);
void default_betas(float* b, int n);
int load_problem(const lmc_problem* p, Problem& q);
int check_prox_prior(const Problem& q, float b);
int check_no_box(const Problem& q, const char* who, const char* why);
int check_no_poisson(const Problem& q, const char* who, const char* why);
int check_poisson(const Problem& q);
int check_no_wl2(const Problem& q, const char* who, const char* why);
int check_wl2(const Problem& q);
int check_no_psf(const Problem& q, const char* who, const char* why);
int check_psf(const Problem& q);
int check_no_spectral(const Problem& q, const char* who, const char* why);
int check_spectral(const Problem& q);
bool wl2_pipe_covers(const lmc::StepArgs& A);       // the full-width pipeline has a weighted form of this launch
bool pois_pipe_covers(const lmc::StepArgs& A);      // the full-width pipeline has a Poisson form of this launch
int make_step_args(const Problem& q, float a, float t, float b, float pt, float s, lmc::StepArgs& A);
void sanitize_pointers(lmc::StepArgs& A);
int variant_of(const Problem& q);
float tol_of(const Problem& q);
// psf: the operator of a launch whose data_kind is LMC_DATA_PSF (with its device table and residual buffer); such a launch without it is not covered
// fft: the same for LMC_DATA_SPECTRAL (with its twiddle table and spectrum buffer)
// wav: the transform of a launch whose prior_kind is LMC_PRIOR_WAVELET_L1 (with its workspace); such a launch without it, or without pxbuf, is not covered
hipError_t launch_step(const lmc::StepArgs& A_in, int variant, hipStream_t st, const char** name, float* state0 = nullptr,
                       float* state1 = nullptr, float* pxbuf = nullptr, const lmc::PsfOp* psf = nullptr, const lmc::WaveletOp* wav = nullptr,
                       const lmc::FftOp* fft = nullptr);

// ---- lmc_solve.hip ----
int cg_solve_fused(const Problem& q, float ts, float* u, const float* rhs, float* r, float* p, float* qq, double* scal,
                   int64_t C, int niter, const float* zero_y, hipStream_t st, float* alt_out = nullptr, float** result = nullptr);

// ---- lmc_tv_exit.hip ----
bool needs_tv_state(const Problem& q);
int tv_prox_rtol(const Problem& q, float pt, const float* x, float* sol, float* tmp, double* obj, int* flag, int64_t n, float* st0, float* st1,
                 hipStream_t st);
int me_tv_prox(const Problem& q, const float* x, float* extra, int64_t n_img, float* state0, float* state1, hipStream_t st, RtState* rt = nullptr);
int tv_prior_rt(const Problem& q, float pt, lmc::StepArgs& A, RtState& rt, float* proxbuf, float* st0, float* st1, hipStream_t st);
int tv_prior_rt_mode(const Problem& q, const lmc::StepArgs& A_probe, float pt);
lmc::EnergyArgs energy_args(const Problem& q);
int pois_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st);
int wl2_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st);
int psf_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st);
int spectral_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, hipStream_t st);     // q.fft carries the buffers
// after launch_energies: g_out = the value of the wavelet prior (nothing for the other priors); q.wav carries the workspace
int wavelet_energy(const Problem& q, const float* x, int64_t n_img, double* g_out, hipStream_t st);
int me_tv_energy(const Problem& q, const float* x, int64_t n_img, double* f_out, float* extra, float* st0, float* st1,
                 double* dbl /* 2*n_img */, hipStream_t st, RtState* rt);

}  // namespace lmc::host

struct lmc_sampler {
  int kind = 0;   // 0 MYULA, 1 ULPDA, 2 MYMALA, 3 SK-ROCK
  int device = -1;   // the device the handle's buffers live on (current at creation); every call on the handle runs there
  // ULPDA state (kind == 1)
  float mu = 0, theta = 1;
  int gfirst = 0, cg_niter = 0, warm = 1;
  const float* z = nullptr;
  float* xhat = nullptr; float* ydual = nullptr; float* uw = nullptr; float* rhs = nullptr;
  float* uw2 = nullptr;       // ULPDA: the other home of the implicit-step solution (two Chebyshev iterations per launch deliver it there)
  float* cr = nullptr; float* cp = nullptr; float* cq = nullptr; float* ctmp = nullptr; float* xi = nullptr;
  float* htb = nullptr; double* scal = nullptr; float* zero_y = nullptr;
  float* tvstate[2] = {nullptr, nullptr};   // dual-state ping-pong for chunked TV proxes (K > 12, ME-TV)
  float* tvwarm[2] = {nullptr, nullptr};    // warm-started TV prox: projected dual (p, q) of the previous / this MYULA iteration, [C][2][H][W]
  int wcur = 0;
  float* extra = nullptr;                   // ME-TV inner prox
  float* pxbuf = nullptr;                   // Haar-l1 prox / early-exit TV prox of the current state
  float* wav_ws = nullptr; double* wav_part = nullptr;    // wavelet prior: the pyramid and the LL ping-pong (1.25 states), the partial sums of its value
  float* psf_tab = nullptr; float* psf_resid = nullptr;   // large PSF: the device tap table (uploaded at creation) and the residual buffer, [C][H][W]
  float* fft_tw = nullptr; float* fft_spec = nullptr; double* fft_part = nullptr;   // spectral data term: twiddle table, spectrum buffer [C][H][Wh] complex, value partials
  float* rtmp = nullptr; double* robj = nullptr; int* rflag = nullptr;   // early-exit TV prox (tv_rtol > 0), pass-by-pass path: pass iterate, objectives, flags
  lmc::host::RtState rt_tv, rt_me;          // early-exit TV prox on the device (tv_prox_rt): of the TV prior / of the ME-TV inner prox
  // launch policy, fixed at creation (lmc_problem fields; their environment variables supply the defaults): see lmc_atomi.h
  int pol_pair = 1;          // 0 never, 1 where it pays, 2 wherever covered: two MYULA iterations per launch (rows kernel)
  int pol_blockpair = 1;     // 0 / 1: two or four iterations per launch on the block kernel
  int pol_overlap = 0;       // 0 by size, 1 on, -1 off
  int pol_bg_wgs = -1;       // workgroups of the background reduction, -1 by size
  lmc::host::Problem prob;
  int C = 0;
  int64_t chain_offset = 0;
  float tau = 0, gamma = 0, epsg = 1;
  uint64_t seed = 0;
  int noise_mode = 0;
  int moments = 0, burn_in = 0, thin = 1;
  int64_t iteration = 0;
  float* x[2] = {nullptr, nullptr};
  float* xspare = nullptr;    // third state array of the two-iterations-per-launch MYULA path (allocated at its first use)
  // kept iterates in between of pair launches whose reductions run on the side stream: arrays of their own, alternating by launch
  float* xmid[2] = {nullptr, nullptr};
  int cur = 0;
  lmc::host::Accumulators acc;          // what the kept iterates are reduced into (lmc_accum.h)
  lmc::StepArgs base{};
  // MYMALA state (kind == 2): proposal mean of the current state, proposal, its mean, energies, decisions
  float* mx = nullptr; float* xp = nullptr; float* mxp = nullptr;
  double* mala_d = nullptr;              // [5C]: U(x), f(x'), g(x'), ||x'-m(x)||^2, ||x-m(x')||^2 ; then [C] log alpha
  int* flag = nullptr;
  unsigned long long* nacc = nullptr;
  bool mala_fresh = false;               // mx / U match x[cur]
  // SK-ROCK state (kind == 3): stage count and the stage coefficients (entry j - 1 = stage j); the third state array of its rotation is xspare
  int sk_stages = 0;
  double sk_mu[LMC_MAX_SKROCK_STAGES] = {}, sk_nu[LMC_MAX_SKROCK_STAGES] = {}, sk_kappa[LMC_MAX_SKROCK_STAGES] = {};
  // lmc_sampler_sapg (allocated at its first call): the per-chain statistic followed by its partial sums, the device traces of theta and gbar,
  // the pinned host-mapped pair (theta_{n+1}, gbar) with its device address, the event recorded after the update kernel
  bool suspend_moments = false;          // the accumulators take nothing while the estimation runs
  double* sapg_stat = nullptr;
  double* sapg_trace = nullptr;
  size_t sapg_trace_n = 0;               // doubles in sapg_trace
  double* sapg_host = nullptr;
  double* sapg_host_dev = nullptr;
  hipEvent_t sapg_ev = nullptr;
  // moment reductions on a side stream, overlapping the next step kernel (HBM-bound reduction under a VALU-bound step kernel); which of them are
  // still running is known only inside one lmc_sampler_step call (SideMoments), which joins them all before it returns
  hipStream_t side = nullptr;
  hipEvent_t side_ev[1 + lmc::host::kSideBatches] = {};   // [0]: "the launch is done" (caller's stream); [1 + i]: "batch i of reductions is done" (side stream)
  std::vector<hipEvent_t> ev;   // pairs (begin, end) around each step-kernel launch of the last step() call
  bool timing = false;
  bool timed = false;
  int last_launches = 0;
  std::string kernel_name;
};

namespace lmc::host {
// ---- lmc_sampler.hip ----
// s->base of a MYULA / MYMALA / SK-ROCK handle from s->prob and the handle's steps, seed and chain ids: the one path of lmc_myula_create and
// lmc_sampler_set_prior_sigma
int rebuild_base(lmc_sampler* s);
// what lmc_sampler_set_prior_sigma and lmc_sampler_sapg refuse (LMC_E_UNSUPPORTED), else LMC_OK
int check_weight_settable(const lmc_sampler* s);
}  // namespace lmc::host
