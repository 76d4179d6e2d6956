// Internals of the C-ABI host code, shared by its translation units (not installed):
//   lmc_capi.hip        the stateless extern "C" entry points, the last error, the per-device workspaces of the stateless calls
//   lmc_problem.hip     lmc_problem -> Problem and its checks, StepArgs of an update, prepare() (which work buffers a problem needs, and the binding
//                       of its operators to them), the step-kernel dispatch, the library defaults
//   lmc_solve.hip       the implicit step (I + ts H^T H) u = rhs: Chebyshev, CG
//   lmc_tv_exit.hip     the early exits of the TV prox, the ME-TV inner prox and envelope, the energies of a problem
//   lmc_sampler.hip     the MYULA, MYMALA, SK-ROCK and ULPDA samplers: create / destroy, state, the step loops
//   lmc_mch.hip         the multi-channel MYULA sampler under the vectorial TV prior (lmc_mch_*): a handle type of its own
//   lmc_sgs.hip         the split Gibbs sampler (lmc_sgs_*): a handle type of its own, its x-draw, coupling and coupling-energy kernels
//   lmc_sapg.hip        the SAPG estimation of the prior weight: its kernels, its stateless calls and lmc_sampler_sapg
//   lmc_accum.hip       the accumulators over the kept samples (lmc_accum.h): their reductions and their set / get / reset entry points
//   lmc_rccl.hip        the dlopen'd RCCL and the all-reduces of the accumulators
// Ownership: this header has the three owners of device memory -- Workspace (problem-dependent work buffers, sized and bound by prepare()), Owned (the
// per-sampler arrays of a handle) and Accumulators (lmc_accum.h).
#pragma once
#include <cmath>
#include <string>
#include <utility>
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
  int data_kind = 0;        // the operator's kind, LMC_DATA_NONE .. LMC_DATA_MASK, LMC_DATA_PSF, LMC_DATA_SPECTRAL, LMC_DATA_RADON, LMC_DATA_SENSE
  lmc::DataTerm term = lmc::kTermL2;     // the data term on that operator (lmc_common.h): Poisson, weighted Gaussian or Huber from LMC_DATA_POISSON_* / _WL2_* / _HUBER_*, and y is
                                         // [2][H][W] then (counts and background, observation and weights, observation and thresholds)
  float sigma_f = 0.f;
  const float* y = nullptr;
  const float* mask = nullptr;
  lmc::BlurTaps taps{};
  lmc::PsfOp psf;           // LMC_DATA_PSF / POISSON_PSF / WL2_PSF / HUBER_PSF: data_kind = LMC_DATA_PSF (with the term), the operator and its device table
  lmc::FftOp fft;           // LMC_DATA_SPECTRAL: the planes at y_dev and the device buffers of whoever owns them
  lmc::RadonOp radon;       // LMC_DATA_RADON / POISSON_RADON / WL2_RADON / HUBER_RADON: data_kind = LMC_DATA_RADON (with the term), y = the sinogram-shaped planes
  lmc::SenseOp sense;       // LMC_DATA_SENSE: n_coils, the descriptor at y_dev and the device buffers of whoever owns them
  int prior_kind = 0;
  float prior_sigma = 0.f;
  lmc::WaveletOp wav;       // LMC_PRIOR_WAVELET_L1: p, levels and the workspace of whoever owns it
  int tgv_niter = 0;        // LMC_PRIOR_TGV: iterations (lmc_problem.tv_niter), alpha0 (eprox_p0) and the step (tv_step; 0: the default) of its prox
  float tgv_alpha0 = 0.f, tgv_step = 0.f;
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

// A device array that grows on demand: it holds at least n elements after need(n); what it held is not kept when it grows.
template <class T>
struct Buf {
  T* p = nullptr;
  size_t n = 0;
  hipError_t need(size_t want) {
    if (want <= n) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, sizeof(T) * want);
    if (e == hipSuccess) n = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
  }
};

// The one owner of the work buffers a problem needs beyond its state arrays.  There is one per device for the stateless entry points (scratch_here: it
// lives for the life of the process; those calls are serialised by the caller, see lmc_atomi.h) and one inside every sampler handle, which never touches
// the other.  prepare() is the one place that decides which buffers a problem needs, grows them and points the problem's operators at them.
struct Workspace {
  Buf<float> state[2];                    // TV dual state ping-pong, [n][4][H][W] each; a chained TGV prox: its state, [n][11][H][W] each
  Buf<float> extra;                       // ME-TV inner prox, [n][H][W]
  Buf<float> prox;                        // a prox formed ahead of the step (Haar-l1, wavelet, closed forms, box, early-exit TV prox), [n][H][W]
  Buf<float> rtmp;                        // pass-by-pass early exit: the iterate of the current pass, [n][H][W]
  // small float64 scratch.  The pass-by-pass early exits lay it out as 2n objectives then n + 1 ints (exit_obj / exit_flag); the ME-TV envelope takes
  // the first 2n doubles, the PSF energy its partial sums, lmc_prior_statistic its segments
  Buf<double> dbl;
  Buf<float> resid;                       // large PSF: the residual rho(H x) of a step, [n][H][W]; Radon operator: rho(A x), [n][n_angles][n_det]; SENSE: the gradient image g, [n][H][W]
  Buf<float> wav;                         // wavelet prior: the thresholded pyramid and the LL ping-pong (1.25 states)
  Buf<double> wav_part;                   // wavelet prior: the partial sums of its value
  Buf<double> vtv_part;                   // vectorial TV: the partial sums of its value (its chained prox carries the dual through state[])
  // large PSF: the device tap table, the pinned host copy it was uploaded from (compared with the next table: equal taps are not uploaded again)
  // and the event behind the last upload (the host copy is not rewritten before that upload has run)
  float* psf_tab = nullptr;
  float* psf_host = nullptr;
  hipEvent_t psf_ev = nullptr;
  bool psf_valid = false;
  // spectral data term: the twiddle table (uploaded once), the spectrum buffer [n][H][Wh] complex, the partial sums of the value
  float* fft_tw = nullptr;
  Buf<float> fft_spec;
  Buf<double> fft_part;
  // Radon operator: the device table (radon_table_floats), the pinned host copy it is uploaded from, the event behind the last upload and what the
  // table was made for (H, W, n_det, then the angles' bits): an equal key is not computed or uploaded again
  float* radon_tab = nullptr;
  float* radon_host = nullptr;
  size_t radon_cap = 0;                   // floats both hold
  hipEvent_t radon_ev = nullptr;
  std::vector<int32_t> radon_key;
  RtState rt_tv, rt_me;                   // device-side early exit of the TV prior's prox / of the ME-TV inner prox
  int tv_exit = -1;                       // the TV prior's early exit as the last prepare() found it: -1 none, else tv_prior_rt_mode (1 fused, 0 prox alone, 2 pass by pass)

  static size_t exit_doubles(size_t n) { return 3 * n + 2; }
  double* exit_obj() const { return dbl.p; }
  int* exit_flag(int64_t n) const { return reinterpret_cast<int*>(dbl.p + 2 * n); }
  // P gets the device table and, with n_resid > 0, the residual buffer.  The table is uploaded in stream order from the pinned copy, and only when it
  // differs from the one held.
  hipError_t bind_psf(lmc::PsfOp& P, size_t n_resid, hipStream_t st);
  // F gets the twiddle table (uploaded once, synchronously: it never changes), the spectrum buffer and the value partials
  hipError_t bind_fft(lmc::FftOp& F, size_t n_spec, size_t n_part);
  // S gets the same twiddle table, spectrum buffer and value partials (the full plane: n_spec = sense_spec_floats) and, with n_g > 0, g in the residual buffer
  hipError_t bind_sense(lmc::SenseOp& S, size_t n_spec, size_t n_g, size_t n_part);
  // R gets the device table of its angles on H x W images and, with n_resid > 0, the residual buffer.  The table is computed on the host and uploaded
  // in stream order from the pinned copy, and only when its key differs from the one held.
  hipError_t bind_radon(lmc::RadonOp& R, int H, int W, size_t n_resid, hipStream_t st);
  // frees the wavelet buffers (the largest a stateless call takes: 1.25 states); the next call that needs them allocates again
  void release_wavelet() { wav.release(); wav_part.release(); }
  void release() {
    for (Buf<float>* b : {&state[0], &state[1], &extra, &prox, &rtmp, &resid, &wav, &fft_spec}) b->release();
    for (Buf<double>* b : {&dbl, &wav_part, &vtv_part, &fft_part}) b->release();
    if (psf_tab) (void)hipFree(psf_tab);
    if (psf_host) (void)hipHostFree(psf_host);
    if (psf_ev) (void)hipEventDestroy(psf_ev);
    if (fft_tw) (void)hipFree(fft_tw);
    psf_tab = psf_host = fft_tw = nullptr; psf_ev = nullptr; psf_valid = false;
    if (radon_tab) (void)hipFree(radon_tab);
    if (radon_host) (void)hipHostFree(radon_host);
    if (radon_ev) (void)hipEventDestroy(radon_ev);
    radon_tab = radon_host = nullptr; radon_ev = nullptr; radon_cap = 0; radon_key.clear();
    rt_tv.release();
    rt_me.release();
    tv_exit = -1;
  }
};
// The workspace of the current device: a process may drive several GPUs (one sampler handle each); the stateless entry points run on the current device.
// Only the stateless extern "C" entry points call it.
Workspace& scratch_here();

// What a sampler handle owns beyond its workspace and accumulators: the per-sampler device arrays, pinned host memory and events.  The handle's fields
// point at them and may rotate; the list frees the original allocations.
struct Owned {
  enum Kind { kDevice, kPinned, kEvent };
  std::vector<std::pair<Kind, void*>> items;
  template <class T>
  hipError_t alloc(T** p, size_t count, bool zero) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, sizeof(T) * count);
    if (e != hipSuccess) return e;
    items.emplace_back(kDevice, *p);
    return zero ? hipMemset(*p, 0, sizeof(T) * count) : hipSuccess;
  }
  template <class T>
  hipError_t pinned(T** p, size_t count, unsigned flags) {
    *p = nullptr;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(p), sizeof(T) * count, flags);
    if (e == hipSuccess) items.emplace_back(kPinned, *p);
    return e;
  }
  hipError_t event(hipEvent_t* ev, unsigned flags) {
    const hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) items.emplace_back(kEvent, *ev);
    return e;
  }
  static void free_item(const std::pair<Kind, void*>& it) {
    if (it.first == kDevice) (void)hipFree(it.second);
    else if (it.first == kPinned) (void)hipHostFree(it.second);
    else (void)hipEventDestroy(static_cast<hipEvent_t>(it.second));
  }
  void drop(void* p) {      // one of them early: an array that a larger one replaces
    for (size_t i = 0; i < items.size(); ++i)
      if (items[i].second == p) { free_item(items[i]); items.erase(items.begin() + i); return; }
  }
  void release() {
    for (const auto& it : items) free_item(it);
    items.clear();
  }
};

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
int check_tgv_step(float step);      // LMC_PRIOR_TGV / lmc_tgv_prox: 0 or a step with 12 step^2 <= 1
int load_problem(const lmc_problem* p, Problem& q);
int check_no_box(const Problem& q, const char* who, const char* why);
// One row per DataTerm, indexed by it (the row of kTermL2 is empty: the plain Gaussian term has no kernels of its own and nothing refuses it)
struct TermInfo {
  const char* name;         // in messages: "the Poisson data term"
  const char* label;        // its kinds in lmc_atomi.h: "LMC_DATA_POISSON_*"
  const char* warm;         // what the warm-started dual lacks for it
  const char *pipe, *pipe_box, *tile, *tile_box;     // the kernel names launch_step reports
  const char *v7_name, *v7_ops;                      // the refusal of step_variant 7: "this <v7_name> problem", "... 5 or 7 taps or <v7_ops>"
};
extern const TermInfo kTerms[lmc::kNumTerms];
// The entry points that have no form of the data term `term` refuse a problem that carries it.
int check_no_term(const Problem& q, lmc::DataTerm term, const char* who, const char* why);
int check_no_psf(const Problem& q, const char* who, const char* why);
int check_no_spectral(const Problem& q, const char* who, const char* why);
int check_no_radon(const Problem& q, const char* who, const char* why);
int check_no_sense(const Problem& q, const char* who, const char* why);
// what the entry points that form the update a x - t grad f + b prox_g (MYULA, MYMALA, SK-ROCK, lmc_fused_eval) refuse: of the anisotropic TV prior
// and of each data term with kernels of its own
int check_step_problem(const Problem& q, float b);
// the first refusal of each of those data terms alone (a non-convex term), for the callers that form no update (lmc_energies)
int check_convex_terms(const Problem& q);
bool term_pipe_covers(const lmc::StepArgs& A);      // the full-width pipeline has a form of this launch's data term (Poisson, weighted, Huber)
int make_step_args(const Problem& q, float a, float t, float b, float pt, float s, lmc::StepArgs& A);
void sanitize_pointers(lmc::StepArgs& A);
int variant_of(const Problem& q);
float tol_of(const Problem& q);
// Grows ws to what the problem q needs on n_img images and points q.psf, q.fft, q.radon, q.sense and q.wav at it (nothing else does: a grown buffer never leaves a
// stale pointer behind).  what: kForStep -- the update `probe` describes (its data term, prior, box and t; pt: its prox parameter) with the proxes that
// run ahead of it; kForEnergyF / kForEnergyG -- f / g of problem_energies.  The stateless calls prepare at every call (no-op once large enough), a
// handle at its creation and never inside lmc_sampler_step.  st: the stream of a PSF table upload.
enum { kForStep = 1, kForEnergyF = 2, kForEnergyG = 4, kForEnergies = kForEnergyF | kForEnergyG };
hipError_t prepare(Workspace& ws, Problem& q, const lmc::StepArgs& probe, int64_t n_img, float pt, int what, hipStream_t st);
// The update A of problem q on the step kernel of `variant`: the dual state and the prox buffer come from ws, the PSF / spectral / Radon / wavelet operators
// from q (bound to ws by prepare; a launch that needs one that is not bound is not covered).
hipError_t launch_step(const lmc::StepArgs& A, int variant, const Problem& q, Workspace& ws, hipStream_t st, const char** name);
inline hipError_t launch_step(const lmc::StepArgs& A, const Problem& q, Workspace& ws, hipStream_t st, const char** name) {
  return launch_step(A, variant_of(q), q, ws, st, name);
}

// ---- lmc_solve.hip ----
int cg_solve_fused(const Problem& q, float ts, float* u, const float* rhs, float* r, float* p, float* qq, double* scal,
                   int64_t C, int niter, const float* zero_y, hipStream_t st, float* alt_out = nullptr, float** result = nullptr);

// ---- lmc_tv_exit.hip ----
bool needs_tv_state(const Problem& q);
// (all of these work in the buffers of ws that prepare() sized for the problem)
// sol <- prox_{pt g}(x) pass by pass; in ws: rtmp, the exit scalars of dbl, the dual state
int tv_prox_rtol(const Problem& q, float pt, const float* x, float* sol, int64_t n, Workspace& ws, hipStream_t st);
// ws.extra <- the inner prox of the ME-TV term at x
int me_tv_prox(const Problem& q, const float* x, int64_t n_img, Workspace& ws, hipStream_t st);
bool me_tv_exit_on_device(const Problem& q, int64_t n_img);     // its early exit (ncvx_rtol > 0) runs on the device, not pass by pass
int tv_prior_rt(const Problem& q, float pt, lmc::StepArgs& A, Workspace& ws, hipStream_t st);
int tv_prior_rt_mode(const Problem& q, const lmc::StepArgs& A_probe, float pt);
// f_out[c] = f(x_c), g_out[c] = g(x_c) of the n_img images at x (either may be NULL): every data term, prior and non-convex term of q
int problem_energies(const Problem& q, const float* x, int64_t n_img, double* f_out, double* g_out, Workspace& ws, hipStream_t st);

}  // namespace lmc::host

namespace lmc::host {
// ---- lmc_accum.hip ----
// The bodies of the accumulator entry points that every handle type with an Accumulators shares (lmc_sampler_*, lmc_sgs_*), after the handle's own
// NULL check and device guard.  moments: the handle was created with moments on.
int accum_get_moments(const Accumulators& a, int moments, double* sum_dev, double* sumsq_dev, uint64_t* count, hipStream_t st);
int accum_set_chain_groups(Accumulators& a, int moments, int32_t n_groups);
int accum_get_group_moments(const Accumulators& a, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, hipStream_t st);
// ---- lmc_sgs.hip ----
// lmc_sgs_xstep behind its entry point: the checks, then the draw with the spectrum buffers of sc
int sgs_xstep(const lmc_problem* prob, const float* z_dev, const float* noise_dev, float* out_dev, int64_t n_img, float rho, Workspace& sc, hipStream_t st);
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
  float* tvwarm[2] = {nullptr, nullptr};    // warm-started TV prox: projected dual (p, q) of the previous / this MYULA iteration, [C][2][H][W]
  int wcur = 0;
  lmc::host::Workspace ws;                  // the work buffers of prob on C images (prepare() at creation; prob's operators point into it)
  lmc::host::Owned own;                     // every other device array, pinned array and event of the handle: the fields below point at its items
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
