/* lmc_atomi.h -- C ABI of the MI355X-native LMC hot path (liblmc_atomi.so).
 *
 * The reference (192459/lmc-atomi) is pure Python and has no FFI: its hot path sits behind
 * duck-typed Python protocols.  This header is the boundary a maintainer of the reference
 * would bind (ctypes stub in INTEGRATION.md); each entry point names the reference
 * interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *  - plain C, no HIP/torch types: `stream` is a hipStream_t passed as void* (NULL = default
 *    stream); pointers ending in _dev are device (HBM) pointers, _host are host pointers.
 *  - every function returns 0 (LMC_OK) or a negative lmc_status; lmc_last_error() gives the
 *    thread-local message of the last failure.  No exception crosses the boundary.
 *  - images are fp32, row-major [H][W] (W fastest); chain states are [C][H][W];
 *    the stacked gradient field is [2][H][W] per image (row-differences first), as the
 *    reference's 2n vectors (algs.py:427).
 *  - the caller owns every buffer it passes; a sampler owns its state/scratch buffers.
 *  - calls on one sampler handle must be serialised by the caller; all work is enqueued on
 *    the given stream; functions that return host values synchronise that stream.
 *  - devices: a sampler lives on the device that is current when it is created and every call on the handle runs there
 *    (the library switches to that device for the duration of the call and restores the caller's; `stream` and the buffers
 *    passed must belong to it).  The stateless operator entry points run on the caller's current device.
 */
#ifndef LMC_ATOMI_H
#define LMC_ATOMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMC_ATOMI_ABI_VERSION 4

typedef enum lmc_status {
  LMC_OK = 0,
  LMC_E_INVALID = -1,     /* bad argument / inconsistent configuration */
  LMC_E_UNSUPPORTED = -2, /* valid request this build has no kernel for */
  LMC_E_HIP = -3,         /* a HIP runtime call failed */
  LMC_E_NOMEM = -4,
  LMC_E_STATE = -5        /* call not allowed in the handle's current state */
} lmc_status;

/* data-fidelity term f(x) = sigma_f/2 * || Op x - y ||^2  (pyproximal.L2 as built at
 * prox_lmc_deconv.py:101-103; same formulae in-repo at algs.py:182-187, 283-288) */
typedef enum lmc_data_kind {
  LMC_DATA_NONE = 0,     /* f = 0 */
  LMC_DATA_IDENTITY = 1, /* Op = I */
  LMC_DATA_BLUR = 2,     /* Op = zero-padded "same" convolution, pylops Convolve2D (prox_lmc_deconv.py:55-69) */
  LMC_DATA_MASK = 3,     /* Op = diag(mask), inpainting (BASELINE config 5) */
  /* Poisson likelihood, y_p ~ Poisson((Op x)_p + beta_p) (additive values; LMC_ATOMI_ABI_VERSION stays 4, the layout of lmc_problem is unchanged).
   * Build-specified (the reference has no such term); this text is its definition.  Operator fields as for kinds 1 to 3; y_dev points to
   * [2][H][W] floats: plane 0 the counts y >= 0 (they need not be integers), plane 1 the known background beta > 0 (a scalar background is a
   * constant plane).  Preconditions, not checked on the device: y >= 0, beta > 0, both finite.  With u = (Op x)_p:
   *   u >= 0:  phi(u) = (u + beta) - y + y log(y / (u + beta))   (0 log 0 = 0)        phi'(u) = 1 - y / (u + beta)
   *   u <  0:  phi(u) = phi(0) + phi'(0) u + y u^2 / (2 beta^2)                       phi'(u) = 1 - y / beta + y u / beta^2
   *   f(x) = sigma_f sum_p phi_p((Op x)_p),   grad f(x) = sigma_f Op^T phi'(Op x)
   * the generalised Kullback-Leibler divergence (the Poisson negative log-likelihood up to a constant) for u >= 0 and its second-order Taylor
   * extension at 0 below: f is convex and C^1 on the whole space (MYULA iterates live near the positive orthant, not in it) with
   * L_f = sigma_f max_p(y_p / beta_p^2) ||Op||^2.  Both branches are one expression: t = 1 / (max(u, 0) + beta), phi'(u) = 1 - y t (1 - t min(u, 0)).
   * sigma_f = 1 is the true likelihood.  Mask: u = m_p x_p, gradient sigma_f m_p phi'(m_p x_p).  A pixel with y_p = 0 has a linear phi, unbounded
   * below as u -> -inf: use the model with box_enable and box_lo = 0.
   * Honoured by lmc_myula_create and lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies and
   * lmc_sampler_energies (f as above: phi in float64 from the fp32 u, summed in float64; every width).  Priors: NONE, L2, L1, EPROX, TV_ISO and
   * TV_ANISO with any tv_niter and tv_lagged_output, box_enable with each as it is honoured for the Gaussian term (so: not by SK-ROCK and SAPG).
   * Kernels: the full-width pipeline (myula_step_pipe_pois_kernel, myula_step_pipe_pois_box_kernel; one team) for the isotropic TV prior with exactly 10
   * dual iterations after tv_lagged_output, W > 128, a separable blur of 5 or 7 taps or a pointwise data term; the LDS-tiled kernel
   * (myula_step_tile_pois_kernel, myula_step_tile_pois_box_kernel) for everything else -- every prior, width and blur.  One iteration per launch
   * (iterations_per_launch is ignored).  LMC_E_UNSUPPORTED, with the reason in lmc_last_error: lmc_mymala_create, lmc_ulpda_create, lmc_l2_prox (no
   * closed implicit step), ncvx_kind != NONE, tv_rtol > 0, tv_warm, LMC_PRIOR_HAAR_L1, a forced step_variant other than 0, 1 and 7; 7 on a problem the
   * pipeline does not cover (from lmc_myula_create / lmc_skrock_create, and from lmc_fused_eval). */
  LMC_DATA_POISSON_IDENTITY = 4,
  LMC_DATA_POISSON_BLUR = 5,
  LMC_DATA_POISSON_MASK = 6,
  /* Per-pixel weights on the Gaussian data term: masked, heteroscedastic deconvolution (additive values; LMC_ATOMI_ABI_VERSION stays 4, the layout of
   * lmc_problem is unchanged: sizeof 200).  Build-specified (the reference has no such term); this text is its definition.  Operator fields as for kinds
   * 1 and 2; y_dev points to [2][H][W] floats: plane 0 the observation y, plane 1 the weights w.  Preconditions, not checked on the device: w >= 0,
   * w and y finite.  With u = (Op x)_p:
   *   f(x) = sigma_f/2 sum_p w_p (u_p - y_p)^2
   *   grad f(x) = sigma_f Op^T( w .* (Op x - y) )
   *   L_f = sigma_f max_p w_p ||Op||^2     (||Op|| <= sum |h| for a blur, 1 for the identity)
   * The weight multiplies the residual BEFORE the adjoint.  w == 1 is kinds 1 and 2.  A pixel with w_p = 0 is unobserved (dead, saturated or masked-out
   * pixels under a blur; w_p = 1 / sigma_p^2 is a noise map; zero weights on a border give the unknown-boundary model).  There is no weighted mask kind:
   * a binary mask m on a blur is w = m, and mask_dev must be NULL with these kinds (LMC_E_INVALID otherwise: a mask would be silently ignored).
   * Honoured by lmc_myula_create, lmc_mymala_create and lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval,
   * lmc_energies and lmc_sampler_energies (u in fp32, w (u - y)^2 widened to and summed in float64; every width).  Priors: NONE, L2, L1, EPROX, TV_ISO
   * and TV_ANISO with any tv_niter and tv_lagged_output, box_enable with each as it is honoured for the unweighted term.  Kernels: the full-width
   * pipeline (myula_step_pipe_wl2_kernel, myula_step_pipe_wl2_box_kernel; one team) for the isotropic TV prior with exactly 10 dual iterations after
   * tv_lagged_output, W > 128, a separable blur of 5 or 7 taps or the identity; the LDS-tiled kernel (myula_step_tile_wl2_kernel,
   * myula_step_tile_wl2_box_kernel) for everything else -- every prior, width and blur.  One iteration per launch (iterations_per_launch is ignored).
   * MYMALA takes f and g of its Metropolis target from the separate energy launch (the weighted pipe kernels form no by-products); its other refusals
   * stand.  LMC_E_UNSUPPORTED, with the reason in lmc_last_error: lmc_ulpda_create, lmc_l2_prox (the implicit step (I + tau sigma_f Op^T W Op)^{-1} is
   * not built), ncvx_kind != NONE, tv_rtol > 0, tv_warm, LMC_PRIOR_HAAR_L1, a forced step_variant other than 0, 1 and 7; 7 on a problem the pipeline
   * does not cover (from the create functions, and from lmc_fused_eval). */
  LMC_DATA_WL2_IDENTITY = 7,
  LMC_DATA_WL2_BLUR = 8,
  /* Large point-spread functions (appended; LMC_ATOMI_ABI_VERSION stays 4): Op = the zero-padded "same" convolution of LMC_DATA_BLUR with a kernel of
   * 1 <= psf_kh, psf_kw <= LMC_MAX_PSF taps and any origin inside it, given by the psf_* fields of lmc_problem and the taps at h_host (kh = kw = oy =
   * ox = 0 with these kinds, LMC_E_INVALID otherwise: the geometry of the small blur is not that of the PSF).  9: the Gaussian term of kind 2; 10: the Poisson term of kinds 4 .. 6 (y_dev = [2][H][W], counts then background);
   * 11: the weighted Gaussian term of kinds 7, 8 (y_dev = [2][H][W], observation then weights; mask_dev must be NULL).  An operator of its own, NOT a
   * larger LMC_DATA_BLUR: the update out = a x - t grad f(x) + b prox(x) + s xi runs as three launches on the caller's stream --
   *   1. r = rho(H x) into a residual buffer (rho(u) = u - y, w (u - y), or the Poisson term's phi'(u)),
   *   2. the step kernel of the same problem WITHOUT a data term: out = a x + b prox(x) + s xi -- every prior, the box, the Philox field and every
   *      forced step_variant as they are for LMC_DATA_NONE (the variant selects the kernel of this launch),
   *   3. out -= t sigma_f H^T r;  a launch without prox and noise (b == 0 and s == 0, e.g. the gradient alone) skips 2 and writes
   *      out = a x - t sigma_f H^T r in 3.
   * Kernels: psf_conv_kernel (lmc_psf.hip), one workgroup per 32 x 64 output tile and image, the tile and its halo staged in LDS, the taps read from a
   * device buffer; a kernel that is an outer product (lmc_psf_separable) runs as two 1-D passes inside the tile unless psf_separable forbids it.
   * Honoured by lmc_myula_create, lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies and
   * lmc_sampler_energies (u in fp32, the terms widened to and summed in float64 by partial sums in a fixed order: equal from run to run).  A sampler
   * handle uploads the taps once and owns the residual buffer; the stateless calls upload in stream order and take the buffer from their scratch.
   * LMC_E_UNSUPPORTED, with the reason in lmc_last_error: lmc_mymala_create, lmc_ulpda_create, lmc_l2_prox (no implicit step, no pinned Metropolis path
   * for it), ncvx_kind != NONE, tv_rtol > 0, tv_warm.  iterations_per_launch is ignored. */
  LMC_DATA_PSF = 9,
  LMC_DATA_POISSON_PSF = 10,
  LMC_DATA_WL2_PSF = 11,
  /* Fourier-domain data term: k-space masks and periodic blurs (appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).  Build-specified;
   * this text is its definition.  F: the unitary 2-D DFT of an H x W real image in numpy's unshifted fft2(norm="ortho") index order; G and b: complex
   * H x W arrays, the gain and the data per frequency.
   *   f(x) = sigma_f / 2 sum_k |G_k (F x)_k - b_k|^2 over the full plane,  grad f(x) = sigma_f Re F^H(conj(G) (G F x - b)),  L_f = sigma_f max_k A_k.
   * x is real, so F x is Hermitian and only the Hermitian part of the residual survives the real part.  With -k = ((-i) mod H, (-j) mod W),
   *   A_k = (|G_k|^2 + |G_-k|^2) / 2 (real),  B_k = (conj(G_k) b_k + G_-k conj(b_-k)) / 2,
   *   grad f = sigma_f irfft2(A rfft2(x) - B) exactly, on the half plane of Wh = W / 2 + 1 columns alone,
   *   prox_{tau f}(v) = irfft2((rfft2(v) + tau sigma_f B) / (1 + tau sigma_f A)),
   *   f = sigma_f / 2 times the half-plane sum of |G_k xh_k - b_k|^2 + |conj(G_-k) xh_k - conj(b_-k)|^2, the second term zeroed in the self-conjugate
   *   columns j = 0 and j = W / 2 (where -k is itself visited): formed from the residuals in fp32, widened to float64 and summed by partial sums in a
   *   fixed order -- never the expanded form A |xh|^2 - 2 Re(.), which cancels.
   * It covers k-space sampling (MRI, gridded radio visibilities: G = mask or sqrt(weights), optionally times a transfer function) and the periodic
   * convolution with a kernel of any support up to the image (G = the unnormalised DFT of the kernel wrapped about its origin, b = F(observation)).
   * The struct has no hole left, so the kind reads only fields that are otherwise unread for it: y_dev -> device floats [11][H][Wh], planes 0 .. 2 =
   * A, Re B, Im B, planes 3 .. 10 = Re / Im of G_k, b_k, conj(G_-k), conj(b_-k), the last two pairs zeroed in the self-conjugate columns
   * (lmc_spectral_tables builds them on the host).  mask_dev, h_host, kh, kw, oy, ox and the psf_* bytes must be NULL / 0 (LMC_E_INVALID otherwise).
   * H and W: powers of two, 8 .. 1024 (LMC_E_UNSUPPORTED otherwise; mixed radix is not built).
   * The update out = a x - t grad f(x) + b prox(x) + s xi runs as LMC_DATA_PSF's does: the spectrum of the residual into a handle-owned buffer
   * (fft_rows_fwd_kernel, fft_cols_spectral_kernel), the step of the same problem without a data term, out -= t sigma_f irfft (fft_rows_inv_kernel);
   * without prox and noise the last launch writes a x - t sigma_f irfft and the middle one is skipped.  Kernels: lmc_fft.hip -- a Stockham autosort in
   * LDS, radix 4 with one radix-2 stage for an odd log2, twiddles from a table computed in float64 and rounded once.
   * Honoured by lmc_myula_create, lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies,
   * lmc_sampler_energies and lmc_l2_prox (the closed form above: niter, warm and the workspace are ignored).  Every prior and box LMC_DATA_NONE takes.
   * A sampler handle owns the spectrum buffer and the twiddle table; the stateless calls take theirs from scratch.  LMC_E_UNSUPPORTED, with the reason
   * in lmc_last_error: lmc_mymala_create, lmc_ulpda_create, ncvx_kind != NONE, tv_rtol > 0, tv_warm.  iterations_per_launch is ignored. */
  LMC_DATA_SPECTRAL = 12,
  /* Huber data term: robust deconvolution with outliers at unknown positions -- impulse noise, cosmic rays, hot or saturated pixels (appended;
   * LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).  Build-specified (the reference has no such term); this text is its definition.
   * Operator fields as for kinds 1 (13), 2 (14) and 9 (15); y_dev points to [2][H][W] floats: plane 0 the observation y, plane 1 the thresholds
   * delta in [0, +inf].  Preconditions, not checked on the device: delta >= 0 and not NaN, y finite.  With u = (Op x)_p and r = u - y_p:
   *   h_delta(r) = r^2 / 2 for |r| <= delta,  delta (|r| - delta / 2) otherwise           psi_delta(r) = h_delta'(r) = clamp(r, -delta, delta)
   *   f(x) = sigma_f sum_p h_delta_p(r_p)
   *   grad f(x) = sigma_f Op^T psi_delta(Op x - y)
   *   L_f = sigma_f ||Op||^2     (psi is 1-Lipschitz: the bound of the plain term; ||Op|| <= sum |h| for a blur, 1 for the identity)
   * The clamp acts on the residual BEFORE the adjoint.  delta_p = +inf is the plain Gaussian term of kinds 1, 2 and 9 at that pixel; delta_p = 0 is an
   * unobserved pixel, so a binary mask on a blur is delta = 0 there: there is no Huber mask kind, and mask_dev must be NULL with these kinds
   * (LMC_E_INVALID otherwise: a mask would be silently ignored).  f is convex and C^1, so the Metropolis target of MYMALA is defined.
   * Honoured by lmc_myula_create and lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies and
   * lmc_sampler_energies -- all three kinds (r in fp32, its branch value widened to and summed in float64; every width) -- and by lmc_mymala_create for
   * kinds 13 and 14, with f and g of the target from the separate energy launch (the Huber pipe kernels form no by-products); kind 15 is refused there
   * like every large PSF.  Priors and box_enable exactly as for the weighted Gaussian term (kinds 7, 8; kind 11 for 15).  Kernels, kinds 13 and 14: the
   * full-width pipeline (myula_step_pipe_hub_kernel, myula_step_pipe_hub_box_kernel; one team) for the isotropic TV prior with exactly 10 dual
   * iterations after tv_lagged_output, W > 128, a separable blur of 5 or 7 taps or the identity; the LDS-tiled kernel (myula_step_tile_hub_kernel,
   * myula_step_tile_hub_box_kernel) for everything else -- every prior, width and blur.  Kind 15: the three launches of LMC_DATA_PSF with
   * r = psi_delta(H x - y) in the first.  One iteration per launch (iterations_per_launch is ignored).  LMC_E_UNSUPPORTED, with the reason in
   * lmc_last_error: lmc_ulpda_create, lmc_l2_prox (no implicit step of the Huber loss under an operator is built), ncvx_kind != NONE, tv_rtol > 0,
   * tv_warm, and for kinds 13 and 14 LMC_PRIOR_HAAR_L1, a forced step_variant other than 0, 1 and 7; 7 on a problem the pipeline does not cover (from the
   * create functions, and from lmc_fused_eval).  Not built: Student-t / Cauchy losses, a weighted Huber term, chained and two-team pipe forms. */
  LMC_DATA_HUBER_IDENTITY = 13,
  LMC_DATA_HUBER_BLUR = 14,
  LMC_DATA_HUBER_PSF = 15,
  /* Tomography: the parallel-beam Radon operator and its data terms (appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).
   * Build-specified (the reference has no projection operator); this text is its definition.
   * Geometry.  Image x[i][j], H x W, row i, column j; pixel centres at X_j = j - (W - 1) / 2 and Y_i = i - (H - 1) / 2.  Angles theta_a, a < n_angles,
   * in radians: the float32 values ARE the angles (the caller rounds once; the tables below are formed from those values widened to double).  The
   * detector has n_det bins at unit spacing.
   * Tables and detector coordinate.  Two tables, computed on the host in float64 and rounded once to float32 (lmc_radon_tables returns them):
   *   ax[a][j] = X_j cos theta_a            by[a][i] = Y_i sin theta_a + (n_det - 1) / 2
   * The detector coordinate of pixel (i, j) at angle a is t = ax[a][j] + by[a][i]: ONE float32 addition, so a checker reproduces t bit for bit.
   * Weight and operator.  w(t, d) = max(0, 1 - |t - d|): the pixel-driven projector with linear interpolation on the detector, evaluated in fp32 as
   * written by one device function that both directions call.
   *   forward  (A x)[a][d]   = sum_{i, j} w(t_{a,i,j}, d) x[i][j]
   *   adjoint  (A^T r)[i][j] = sum_a sum_{d in {floor(t), floor(t) + 1}, 0 <= d < n_det} w(t, d) r[a][d]
   * Bins outside the detector are dropped in both directions: a detector narrower than the image is a valid, truncated operator.  Sinograms are
   * [n_img][n_angles][n_det] floats.  Results are deterministic: both directions gather, in a fixed summation order, without atomics.
   * Limits: 1 <= n_angles <= LMC_MAX_RADON_ANGLES, 1 <= n_det <= LMC_MAX_RADON_DET (LMC_E_INVALID otherwise); H, W up to LMC_MAX_RADON_SIDE each
   * (LMC_E_UNSUPPORTED beyond: the forward kernel's fp32 estimate of the pixels that reach a bin is proved to that size).
   * Data terms, with u = A x in the sinogram domain; the formulas of kinds 4 .. 8 and 13 .. 15 carry over word for word with Op = A:
   *   16  Gaussian            f = sigma_f / 2 sum (u - y)^2            y_dev = [n_angles][n_det]
   *   17  Poisson             kinds 4 .. 6                             y_dev = [2][n_angles][n_det]: counts, background
   *   18  weighted Gaussian   kinds 7, 8                               y_dev = [2][n_angles][n_det]: observation, weights
   *   19  Huber               kinds 13 .. 15                           y_dev = [2][n_angles][n_det]: observation, thresholds
   * The struct has no hole left, so the kinds read fields that are otherwise unread for them: kh = n_angles, kw = n_det, h_host = the n_angles angles
   * (host floats, copied by the callee).  oy, ox, the psf_* bytes, psf_separable and mask_dev must be 0 / NULL (LMC_E_INVALID otherwise); a non-finite
   * angle is LMC_E_INVALID.
   * Lipschitz bound.  A is non-negative, so ||A||^2 <= max(A 1) max(A^T 1), and max(A^T 1) <= n_angles; L_f is the term's own factor (1, max(y /
   * beta^2), max(w), 1) times sigma_f times that product.
   * The update out = a x - t grad f(x) + b prox(x) + s xi runs as LMC_DATA_PSF's does: r = rho(A x) into a handle-owned sinogram buffer
   * (radon_fwd_kernel), the step of the same problem without a data term -- every prior, the box, the Philox field and every forced step_variant as
   * they are for LMC_DATA_NONE --, out -= t sigma_f A^T r (radon_adj_kernel); without prox and noise the last launch writes a x - t sigma_f A^T r
   * and the middle one is skipped.  Kernels: lmc_radon.hip -- forward: a workgroup owns 256 bins and 8 angles, the image passes through LDS band by band
   * and a lane evaluates w on the four pixels of each row (or column, by the angle) that can reach its bin; adjoint: a lane owns a pixel and walks the
   * angles.  Honoured by lmc_myula_create, lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies and
   * lmc_sampler_energies (u in fp32, the terms widened to and summed in float64 by partial sums in a fixed order).  A sampler handle owns the tables
   * and the residual buffer; the stateless calls take theirs from scratch.  LMC_E_UNSUPPORTED, with the reason in lmc_last_error: lmc_mymala_create,
   * lmc_ulpda_create, lmc_l2_prox, ncvx_kind != NONE, tv_rtol > 0, tv_warm.  iterations_per_launch is ignored.  Not built: fan and cone beams, a
   * detector spacing other than 1 and detector offsets, ray-driven or distance-driven footprints, filtered back-projection, a fused form. */
  LMC_DATA_RADON = 16,
  LMC_DATA_POISSON_RADON = 17,
  LMC_DATA_WL2_RADON = 18,
  LMC_DATA_HUBER_RADON = 19,
  /* Multi-coil MRI: the SENSE data term (appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).  Build-specified; this text is its
   * definition.  x: a real H x W image.  S_c: complex H x W sensitivity maps, c < n_coils (they carry the phase, which is why x is real).  M: a real
   * H x W k-space weight, M >= 0 -- a binary sampling mask or sqrt(density weight).  b_c: complex H x W data per coil.  F: the unitary 2-D DFT in
   * numpy's unshifted fft2(norm="ortho") order, over the full plane.
   *   e_c      = M . F(S_c . x) - b_c
   *   f(x)     = sigma_f / 2 sum_c sum_k |e_c,k|^2
   *   grad f   = sigma_f sum_c Re[ conj(S_c) . F^H( M . e_c ) ]
   *   L_f      = sigma_f max_k M_k^2 max_p sum_c |S_c(p)|^2          (F is unitary: ||M F S_c x|| <= max M ||S_c x||)
   * The value is formed from the residuals e_c in fp32, widened to float64 and summed by partial sums in a fixed order -- never the expanded form.  Coils
   * are summed in the order c = 0, 1, ...
   * The struct has no hole left, so the kind reads fields that are otherwise unread for it: kh = n_coils, 1 .. LMC_MAX_COILS (LMC_E_INVALID otherwise);
   * y_dev -> device floats [1 + 4 n_coils][H][W]: plane 0 = M; planes 1 + 2c, 2 + 2c = Re S_c, Im S_c; planes 1 + 2 n_coils + 2c and the next = Re b_c,
   * Im b_c.  mask_dev, h_host, kw, oy, ox and the psf_* bytes must be NULL / 0 (LMC_E_INVALID otherwise).  H and W: powers of two, 8 .. 1024
   * (LMC_E_UNSUPPORTED otherwise; mixed radix is not built).  Preconditions, not checked on the device: M >= 0, everything finite.
   * The update out = a x - t grad f(x) + b prox(x) + s xi runs as LMC_DATA_SPECTRAL's does: the whole gradient image g = sum_c Re[conj(S_c) F^H(M e_c)]
   * at x into a handle-owned real buffer [C][H][W] -- per coil sense_rows_fwd_kernel, sense_cols_kernel, sense_rows_inv_kernel (store for coil 0, add
   * after it) through one spectrum buffer [C][H][W] complex --, the step of the same problem without a data term, then the elementwise
   * out -= t sigma_f g (sense_axpy_kernel); without prox and noise the last launch writes a x - t sigma_f g and the middle one is skipped.  Kernels:
   * lmc_sense_kernel.h around the LDS transforms of LMC_DATA_SPECTRAL; no atomics, equal bits from run to run.
   * Honoured by lmc_myula_create, lmc_skrock_create with all of lmc_sampler_* (lmc_sampler_sapg included), lmc_fused_eval, lmc_energies and
   * lmc_sampler_energies.  Every prior and box LMC_DATA_NONE takes.  A sampler handle owns the spectrum buffer, g and the twiddle table; the stateless
   * calls take theirs from scratch.  LMC_E_UNSUPPORTED, with the reason in lmc_last_error: lmc_mymala_create, lmc_ulpda_create, lmc_l2_prox (the implicit
   * step is diagonal in neither domain), lmc_sgs_create (the x-draw has no closed form), lmc_mch_create, ncvx_kind != NONE, tv_rtol > 0, tv_warm.
   * iterations_per_launch is ignored.  Not built: complex-valued images, the estimation of the maps, non-Cartesian trajectories, other sides, several
   * coils per launch, a half-plane form for real maps. */
  LMC_DATA_SENSE = 20
} lmc_data_kind;

/* prior g whose prox enters the MYULA update (algs.py:569) */
typedef enum lmc_prior_kind {
  LMC_PRIOR_NONE = 0,   /* prox = identity */
  LMC_PRIOR_L2 = 1,     /* g = sigma/2 ||x||^2      : prox_t = x / (1 + t*sigma)          */
  LMC_PRIOR_L1 = 2,     /* g = sigma ||x||_1        : soft threshold t*sigma  (prox.py:18) */
  LMC_PRIOR_TV_ISO = 3, /* g = sigma TV_iso(x)      : tv_niter FGP dual iterations (pyproximal.TV, prox_lmc_deconv.py:122);
                         *  in ULPDA: g o A with g = sigma*L21 (prox_lmc_deconv.py:116), dual prox = l2-ball projection */
  LMC_PRIOR_TV_ANISO = 4, /* g = sigma (||d_r x||_1 + ||d_c x||_1), the anisotropic TV (build-specified: pyproximal.TV has no such form).
                           *  MYULA, MYMALA, lmc_fused_eval: prox by tv_niter FGP dual iterations with the dual clipped to [-1, 1] per component
                           *  (tv_step, tv_betas_host, tv_lagged_output as for LMC_PRIOR_TV_ISO); tv_niter in 1..LMC_MAX_TV_ITERS, else
                           *  LMC_E_INVALID; tv_rtol > 0, tv_warm and prox_scale: LMC_E_UNSUPPORTED (no early exit, no warm dual for it).  Kernels:
                           *  the full-width pipeline for tv_niter in {10, 20, ... 60} on images wider than 128 columns (any alignment; column
                           *  strips above 512), the LDS-tiled kernel elsewhere.  lmc_energies: g as above.
                           *  In ULPDA: g o A with g = sigma*L1 (prox_lmc_deconv.py:119), dual prox = clip; tv_niter may stay 0 there and
                           *  for lmc_energies. */
  LMC_PRIOR_HAAR_L1 = 5, /* g = sigma * || detail coefficients of the 3-level orthonormal Haar transform of x ||_1 (BASELINE
                          * config 5; no counterpart in the reference): prox = W^T soft(W x, t*sigma); H, W multiples of 8 */
  LMC_PRIOR_EPROX = 6,   /* (ABI 3) a separable prior whose prox is one of the closed forms of prox.py (lmc_eprox_kind below; prox.py:18-85, used
                          * inside the reference's samplers at prox_lmc.py:106,115): prox(x) = prox_X(x; p0, p1) pixel by pixel, evaluated inside
                          * the fused step kernel.  lmc_problem.eprox_kind / eprox_p0 / eprox_p1; eprox_scale_mask bit i set = parameter i is
                          * multiplied by the prox parameter (epsg * gamma in MYULA) -- e.g. prox_laplace(x, gamma * lam): p0 = lam, mask = 1.
                          * MYULA steps and lmc_fused_eval; its value g(x) is not defined for every family: lmc_energies returns g = 0.
                          * lmc_mymala_create returns LMC_E_UNSUPPORTED for it: without a value of g the Metropolis target exp(-f - epsg*g) is
                          * undefined (lmc_prior_statistic and lmc_sampler_sapg refuse it for the same reason). */
  /* Daubechies wavelet-l1 prior (appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).  Build-specified; this text is its definition.
   * p in 1 .. 4 vanishing moments, L in 1 .. LMC_MAX_WAVELET_LEVELS levels.  The kind reads its two parameters from fields that are otherwise unread
   * for it (the struct has no hole left):  tv_niter = L (levels),  eprox_kind = p;  prior_sigma = sigma.
   *   scaling filter h[0 .. 2p-1]: the extremal-phase (minimum-phase) Daubechies filter -- P(y) = sum_{k<p} C(p-1+k, k) y^k with y = (2 - z - 1/z)/4, of
   *   every root pair {z, 1/z} the root inside the unit circle, times (1 + z)^p, normalised to sum h = sqrt 2 (db2 = 0.48296291, 0.83651630,
   *   0.22414387, -0.12940952; lmc_wavelet_filter returns the compiled-in taps);  wavelet filter g[k] = (-1)^k h[2p-1-k].
   *   one level on a periodic signal a of even length n >= 2p:  lo[m] = sum_k h[k] a[(2m+k) mod n],  hi[m] = sum_k g[k] a[(2m+k) mod n],  m < n/2.
   *   2-D: one level along the rows, then along the columns (subbands LL, and the three details), deeper levels on LL; W over L levels is orthonormal.
   *   g(x) = sigma * sum |all detail coefficients of all levels| (the last LL is not penalised);  prox_{t g}(x) = W^T S(W x), S the soft threshold
   *   t sigma on the details -- exact, no inner iteration.  p = 1, L = 3 is the value and prox of LMC_PRIOR_HAAR_L1 (other kernels, other rounding).
   * Preconditions (LMC_E_INVALID otherwise): H and W multiples of 2^L, min(H, W) >> (L - 1) >= 2p (every level wraps at most once).
   * Kernels (lmc_wavelet.hip): one launch per level and direction, wav_fwd_kernel / wav_inv_kernel, the tile and its halo in LDS, the threshold fused
   * into the stores of the forward levels; the prox goes to a buffer the fused step kernel then consumes as a ready-made prox (the route of
   * LMC_PRIOR_HAAR_L1: the step kernel is that of the same problem with LMC_PRIOR_NONE), so every data term, the Poisson and weighted Gaussian terms
   * and the large PSF included, takes it.  Workspace: 1.25 state-sized buffers (the thresholded pyramid, the LL ping-pong), owned by the sampler handle
   * or taken from the scratch of the stateless calls.  The value is formed by partial sums in a fixed order: equal from run to run.
   * Honoured by lmc_myula_create, lmc_mymala_create, lmc_skrock_create, lmc_fused_eval, lmc_energies, lmc_sampler_energies, lmc_prior_statistic,
   * lmc_sapg_dimension (d = H W - (H >> L)(W >> L), k = 1), lmc_sampler_sapg, lmc_sampler_set_prior_sigma.  LMC_E_UNSUPPORTED, with the reason in
   * lmc_last_error: box_enable (not separable, as LMC_PRIOR_HAAR_L1), prox_scale, lmc_ulpda_create.  iterations_per_launch is ignored. */
  LMC_PRIOR_WAVELET_L1 = 7,
  /* Vectorial total variation of a multi-channel image (appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).  Build-specified (the
   * reference has single-plane images only); this text is its definition.  On x[ch][H][W], ch = 0 .. n_channels - 1, 1 <= n_channels <= LMC_MAX_CHANNELS:
   *   g(x) = sigma * VTV(x),   VTV(x) = sum_pixels sqrt( sum_ch (d_r x_ch)^2 + (d_c x_ch)^2 )
   * -- ONE gradient norm per pixel over all channels (Blomgren-Chan / Bresson-Chan, the "Frobenius" form), with the forward differences of lmc_gradient
   * (zero in the last row / column) and their negative adjoint div.  The channels share their edges; they couple in the dual projection and nowhere else.
   * prox_{t g}(x) is niter fast-gradient-projection dual iterations from the zero dual with gamma = t sigma -- the loop of LMC_PRIOR_TV_ISO with the
   * projection weight shared by the channels of a pixel:
   *   (rr, ss) = (p, q) = 0                                          per channel
   *   repeat niter times (k = 0 ...):
   *     sol_ch = clip(x_ch - gamma div(rr_ch, ss_ch))                clip only with a box; else the identity
   *     (r, s)_ch = (rr, ss)_ch - (step / gamma) grad(sol_ch)
   *     w = max(1, sqrt(sum_ch r_ch^2 + s_ch^2))                     ONE w per pixel
   *     (p', q')_ch = (r, s)_ch / w
   *     (rr, ss)_ch = (p', q')_ch + beta_k ((p', q')_ch - (p, q)_ch);   (p, q) = (p', q')
   *   return clip(x_ch - gamma div(rr_ch, ss_ch))
   * step defaults to 1/8 (||grad||^2 <= 8 holds per channel and the operator is block-diagonal over the channels); beta_k: the table of LMC_PRIOR_TV_ISO.
   * With a box the primal iterate of EVERY dual iteration and the returned one are clipped (Beck and Teboulle's constrained FGP, as the box TV kernels do it;
   * clipping afterwards gives a different point).  n_channels = 1 is LMC_PRIOR_TV_ISO.  1 <= niter <= LMC_MAX_TV_ITERS.
   * Layout: channel-major -- image (ch, n) is at x + ch * channel_stride + n * H * W; a batch of n_img multi-channel images has channel_stride = n_img * H * W.
   * Kernels (lmc_vtv.hip): vtv_prox_kernel -- a workgroup owns a patch (tile + halo) of one multi-channel image, a lane all channels of its pixels, so w is
   * lane-local; up to 10 dual iterations are ONE launch, more are chained launches that carry the dual state through work buffers exactly.  vtv_value_kernel:
   * float64 partial sums in a fixed order.  No atomics: equal runs give equal bits.
   * Valid in lmc_mch_* and lmc_vtv_* only; every other entry point that takes an lmc_problem: LMC_E_UNSUPPORTED with the reason in lmc_last_error
   * (lmc_prior_statistic and lmc_sapg_dimension, which read the kinds with a single-plane value alone, keep their range check: LMC_E_INVALID). */
  LMC_PRIOR_VTV = 8,
  /* Total generalised variation of order two (Bredies, Kunisch and Pock 2010; appended; LMC_ATOMI_ABI_VERSION stays 4 and sizeof(lmc_problem) 200).
   * Build-specified (the reference has first-order TV only); this text is its definition.
   * Operators.  grad: the forward differences of lmc_gradient, zero in the last row / column; div: their negative adjoint.  For a field w = (w1, w2):
   *   E w = (e11, e22, e12) with (e11, a) = grad w1, (b, e22) = grad w2, e12 = (a + b) / 2 -- the symmetrised derivative;
   *   |e|_F = sqrt(e11^2 + e22^2 + 2 e12^2), the Frobenius norm of the symmetric 2 x 2 matrix;
   *   div2 q = (div(q11, q12), div(q12, q22)), so that <E w, q>_F = -<w, div2 q>.
   * The prior:
   *   g(x) = sigma * min_w ( sum_pixels |grad x - w|_2 + alpha0 * sum_pixels |E w|_F )
   * An affine ramp costs nothing (w = grad x, E w = 0) where TV charges its full variation: no staircase in the samples.
   * The prox at parameter t: lam1 = t sigma, lam0 = alpha0 lam1.  prox_{t g}(v) is niter Chambolle-Pock iterations on the saddle-point problem
   * min_{u, w} max_{|p| <= lam1, |q|_F <= lam0} 1/2 |u - v|^2 + <grad u - w, p> + <E w, q>, from u = ub = v and w = wb = p = q = 0, with ONE step s
   * for both sides:
   *   p  <- P_lam1( p + s (grad ub - wb) )           P_lam(z) = z / max(1, |z| / lam) per pixel; for q the norm is |.|_F above
   *   q  <- P_lam0( q + s E wb )
   *   u' = clip( (u + s div p + s v) / (1 + s) )     clip only with a box: the exact prox of 1/2 |. - v|^2 + the indicator (clipping after the loop
   *                                                  gives a different point)
   *   w' = w + s (p + div2 q)
   *   ub = 2 u' - u,  wb = 2 w' - w,  (u, w) = (u', w')
   *   return u
   * s defaults to 1 / sqrt(12): ||K||^2 < 12 for K = [[grad, -I], [0, E]] (power iteration on 64 x 64 gives 11.34); a step with 12 s^2 > 1 (beyond
   * float32 rounding of the default) is LMC_E_INVALID.  The count is fixed and the result is the TRUNCATED iterate, as LMC_PRIOR_TV_ISO's is: the
   * iteration converges sublinearly (on a 32 x 48 two-facet affine image with noise of sd 10 at lam1 = 5 the distance to the converged prox relative to
   * |prox - v| is 0.14, 0.085, 0.048, 0.032, 0.021 after 10, 20, 40, 80, 160 iterations).
   * Fields, read from slots the kind does not otherwise use (the struct has no hole left):  prior_sigma = sigma;  tv_niter = niter, 1 .. LMC_MAX_TGV_ITERS;
   * eprox_p0 = alpha0, finite and > 0;  tv_step = s, 0 selects the default;  box_* as for LMC_PRIOR_TV_ISO.  Anything else: LMC_E_INVALID.
   * Kernel (lmc_tgv.hip): tgv_prox_kernel -- a workgroup owns a 64 x 64 patch (tile + halo) of one image, a lane v, u, w, p, q of its four pixels in
   * registers; the fields neighbours read (ub, wb at +1; p, q at -1) live in LDS, eight planes.  lmc_tgv_launch_iters() iterations are ONE launch (its halo);
   * more are chained launches that carry (u, ub, w, wb, p, q), 11 planes, through two work buffers exactly.  Two barriers per iteration, no atomics:
   * equal runs give equal bits.  The prox goes to a buffer that the step kernel of the same problem WITHOUT a prior consumes as a ready-made prox (the
   * route of LMC_PRIOR_WAVELET_L1), so every data term -- blur, mask, Poisson, weighted, Huber, large PSF, spectral, Radon -- and the box take it.
   * Honoured by lmc_myula_create, lmc_skrock_create (not with a box, as every prior) and lmc_fused_eval.  lmc_energies and lmc_sampler_energies report
   * g = 0 (the LMC_PRIOR_EPROX precedent): the value is a minimisation over w and is not built.  LMC_E_UNSUPPORTED, with the reason in lmc_last_error:
   * lmc_mymala_create, lmc_ulpda_create, lmc_mch_create, lmc_sampler_sapg, lmc_sampler_set_prior_sigma, lmc_prior_statistic, lmc_sapg_dimension (all
   * need the value or a dual form); prox_scale, tv_rtol > 0, tv_warm, tv_lagged_output.  iterations_per_launch is ignored.  Not built: the value, a dual
   * carried across sampler iterations, a prox fused into the step kernel, TGV of higher order, vectorial TGV. */
  LMC_PRIOR_TGV = 9
} lmc_prior_kind;

typedef enum lmc_ncvx_kind {
  LMC_NCVX_NONE = 0,
  LMC_NCVX_MC_TV = 1,   /* minimax-concave TV (Moreau envelope of l1 composed with the gradient), isotropic */
  LMC_NCVX_ME_TV = 2,   /* Moreau envelope of isotropic TV itself (Op2 = None): grad env = (x - prox_{gamma TV}(x))/gamma,
                         * prox by ncvx_niter FGP iterations (niter_l2 = 50 at prox_lmc_deconv.py:111; algs.py:169,282) */
  LMC_NCVX_MC_TV_ANISO = 3,  /* the anisotropic MC-TV branches (isotropic = False, Op2 = gradient; algs.py:218-219, 278-279): the Moreau
                              * envelope of l1 on every component of the gradient: grad = A^T clip(A x / gamma, -1, 1) */
  LMC_NCVX_ME_TV_ANISO = 4   /* (ABI 3) the anisotropic ME-TV branch (isotropic = False, Op2 = None; algs.py:170): the Moreau envelope of the 1-D TV of
                              * the FLATTENED image (row-major, differences across row ends included), inner prox by ncvx_niter 1-D FGP iterations with
                              * the early exit ncvx_rtol.  Plain coverage (one pass over the images per dual iteration; with ncvx_rtol > 0 the host reads
                              * a counter after every pass): no model of the reference's driver uses it. */
} lmc_ncvx_kind;

typedef enum lmc_noise_mode {
  LMC_NOISE_PHILOX = 0,   /* counter-based Philox4x32-10 + Box-Muller, keyed by (seed, iteration, global chain, pixel) */
  LMC_NOISE_INJECTED = 1, /* caller supplies xi (parity tests: replaces algs.py:565) */
  LMC_NOISE_NONE = 2
} lmc_noise_mode;

#define LMC_MAX_BLUR 9       /* kernels up to 9x9 */
#define LMC_MAX_PSF 33       /* LMC_DATA_PSF / lmc_psf_apply: kernels up to 33x33 (a Gaussian of sigma = 5 px at +-3 sigma; an even kernel of 32) */
#define LMC_MAX_TV_ITERS 64
#define LMC_MAX_SKROCK_STAGES 64
#define LMC_MAX_CHAIN_GROUPS 64
#define LMC_MAX_COV_PROBES 32
#define LMC_MAX_WAVELET_LEVELS 8   /* LMC_PRIOR_WAVELET_L1: levels of the transform */
#define LMC_MAX_RADON_ANGLES 1024  /* LMC_DATA_RADON .. LMC_DATA_HUBER_RADON / lmc_radon_apply: projection angles */
#define LMC_MAX_RADON_DET 4096     /* ... detector bins */
#define LMC_MAX_RADON_SIDE 1048576 /* ... image rows, image columns */
#define LMC_MAX_CHANNELS 4         /* LMC_PRIOR_VTV: channels of a multi-channel image */
#define LMC_MAX_TGV_ITERS 256      /* LMC_PRIOR_TGV: primal-dual iterations of the prox */
#define LMC_MAX_COILS 32           /* LMC_DATA_SENSE / lmc_sense_apply: receive coils */

/* Geometry + potential U(x) = f(x) + eps*g(x).  Plain data; copied by the callee. */
typedef struct lmc_problem {
  uint32_t struct_size;     /* = sizeof(lmc_problem) */
  int32_t H, W;
  /* data term */
  int32_t data_kind;        /* lmc_data_kind */
  float sigma_f;            /* multiplies the L2 term: 1/sigma^2 at prox_lmc_deconv.py:101 */
  /* Large PSF: read with LMC_DATA_PSF / POISSON_PSF / WL2_PSF / HUBER_PSF only.  The kernel's size, 1 .. LMC_MAX_PSF each, and its origin (pylops `offset`) inside it;
   * the psf_kh * psf_kw taps, row-major, are at h_host (copied by the callee).  Bad geometry: LMC_E_INVALID.  The four bytes fill the alignment hole in
   * front of y_dev and psf_separable (below) the one in front of prox_scale: no field moves and sizeof(lmc_problem) stays 200, so LMC_ATOMI_ABI_VERSION
   * stays 4 and a caller built against the earlier header is unaffected (it never sets these kinds). */
  uint8_t psf_kh, psf_kw, psf_oy, psf_ox;
  const float* y_dev;       /* [H][W] observation (borrowed; must outlive every use) */
  const float* mask_dev;    /* [H][W], LMC_DATA_MASK only */
  int32_t kh, kw, oy, ox;   /* LMC_DATA_BLUR: kernel size and origin (pylops `offset`); 0 with the large-PSF kinds; the Radon kinds: kh = n_angles, kw = n_det, oy = ox = 0 */
  const float* h_host;      /* kh*kw taps, row-major, host memory (large-PSF kinds: psf_kh*psf_kw taps; the Radon kinds: the n_angles angles in radians) */
  /* prior */
  int32_t prior_kind;       /* lmc_prior_kind */
  float prior_sigma;        /* multiplicative coefficient of g (tau_reg = 0.3 at prox_lmc_deconv.py:116-122) */
  int32_t tv_niter;         /* LMC_PRIOR_TV_ISO: number of dual iterations (niter_tv = 10); LMC_PRIOR_WAVELET_L1: the levels of the transform */
  float tv_step;            /* dual step is tv_step / (prox parameter); 0 -> 1/8 */
  const float* tv_betas_host; /* tv_niter momentum coefficients, host; NULL -> UNLocBoX/pyproximal sequence */
  /* non-log-concave data term of algs.L2_ncvx_tv (algs.py:22-291): f(x) = sigma_f/2||Hx-y||^2 - ncvx_lambda * env_gamma(TV)(x).
   * LMC_NCVX_MC_TV: Op2 = gradient, isotropic (algs.py:273-277): grad f = sigma_f H^T(Hx-y) - lambda * A^T( A x / max(|A x|, gamma) ) */
  int32_t ncvx_kind;        /* lmc_ncvx_kind */
  float ncvx_lambda;        /* lamda (= tau_reg at prox_lmc_deconv.py:106) */
  float ncvx_gamma;         /* gamma (= gamma_mc = gamma_me = 15 at prox_lmc_deconv.py:40,106,111) */
  int32_t ncvx_niter;       /* LMC_NCVX_ME_TV: dual iterations of the inner TV prox */
  /* ---- ABI 2 ---- */
  /* Which truncated iterate the TV prox returns.  pyproximal.TV.prox forms `sol = x - gamma div(r, s)` at the TOP of each loop pass and
   * returns the `sol` of the pass it leaves in; whether a run of `niter` reflects niter or niter - 1 dual updates depends on the loop
   * bound of the (un-vendored, un-pinned) upstream version -- it cannot be settled in this image.
   * 0 (default): after tv_niter dual updates; 1: after tv_niter - 1 ("lagged": one pipeline stage fewer).  Applies to the
   * LMC_PRIOR_TV_ISO prox and to the inner prox of the ME-TV term. */
  int32_t tv_lagged_output;
  /* pyproximal.TV's per-image early exit on the relative change of the primal objective (its default rtol = 1e-4, which the reference's
   * call at prox_lmc_deconv.py:122 does not override): at the top of loop pass j >= 1 the iterate x - gamma div(r_j) is returned when
   * |obj_j - obj_{j-1}| / obj_j < rtol.  0 (default): off -- every image runs tv_niter dual iterations in one fused launch.  > 0: every image
   * (chain) leaves in the pass the reference's loop leaves it in.  Two implementations, chosen by tv_exit_path:
   *  - on the device, without synchronisation (ABI 3; the default where the full-width pipeline covers the problem: every width
   *    128 < W <= 16384, rows of any alignment, tv_niter <= 60; images wider than 512 columns run as column strips whose workgroups
   *    add their shares of a chain's objectives): the fused launch runs every chain with a PREDICTED pass count
   *    (the pass it left in at the previous call), the stages past it hand the dual through, and the primal objectives of all the iterates
   *    formed are by-products; a one-thread-per-chain kernel replays the exit test on them and the chains whose prediction was wrong
   *    run again (at most three more rounds settle every chain; the launches of settled chains return at once).
   *  - pass by pass (ABI 2; everything else -- W <= 128, tv_niter > 60 -- and tv_exit_path = 1): one launch per loop pass for the iterate, one for its objective; the host reads the number
   *    of images still iterating after every pass, so this path SYNCHRONISES the stream.
   * Not with tv_warm or MYMALA. */
  float tv_rtol;
  /* Step-kernel variant for launches configured from this problem: 0 = the library default (lmc_set_step_variant, itself "auto"
   * unless changed), 1..8 as listed at lmc_set_step_variant. */
  int32_t step_variant;
  /* Relative residual |r| <= tol |b| of the implicit data step (lmc_l2_prox, ULPDA): 0 = the library default
   * (lmc_set_cg_tolerance, itself 1e-6 unless changed), > 0 explicit, < 0 disabled (always all iterations, CG). */
  float implicit_tol;
  /* MYULA samplers only (build extension; NOT the reference's algorithm, whose pyproximal.TV.prox starts every call from a zero dual):
   * != 0 carries the projected TV dual (p, q) from one MYULA iteration to the next -- tv_niter in {1, 2, 3} dual iterations per
   * MYULA iteration, momentum restarted, +16 B per pixel and iteration of HBM traffic for the dual field.  SURVEY section 8(d) "K in
   * {1,3} warm-dual reported too".  lmc_sampler_set_state resets the dual to zero.  Needs the full-width pipeline kernel
   * (W > 128, W % 4 == 0 up to 256 columns and W % 8 == 0 above; separable blur / pointwise / no data term), otherwise LMC_E_UNSUPPORTED. */
  int32_t tv_warm;
  /* ---- ABI 3 ---- */
  /* The same early exit for the inner prox of the ME-TV term: algs.L2_ncvx_tv builds it as TV(dims, 1., niter, rtol) with the class's own
   * default rtol = 1e-4 (algs.py:130,169), used by value, gradient and prox of models M3 / M6 / M9 (prox_lmc_deconv.py:111-113).
   * 0: fixed ncvx_niter updates.  > 0: the device path above over the chained launches (ncvx_niter <= 60, same widths); elsewhere
   * (W <= 128, ncvx_niter > 60, tv_exit_path = 1) the pass-by-pass path above, which synchronises the stream after every pass. */
  float ncvx_rtol;
  int32_t tv_exit_path;           /* tv_rtol > 0: 0 = the device path where it covers the problem, 1 = always pass by pass (synchronises) */
  /* Launch policy of samplers created from this problem (0 = the library decides).  Each field has an environment variable that supplies the
   * process-wide default when the field is 0; both are read ONCE, when the sampler is created -- never inside lmc_sampler_step.
   *  iterations_per_launch  (LMC_ITERS_PER_LAUNCH, and the older LMC_ROWS_PAIR / LMC_BLOCK_PAIR / LMC_CHEB_PAIR): 0 = several iterations per
   *      launch where a kernel covers the configuration and the launch is large enough to pay (two MYULA iterations: separable 5 x 5 box +
   *      closed-form prior, mask + Haar; two Chebyshev iterations of the implicit step); 1 = always one; 2 = wherever covered (tests).
   *  moments_overlap  (LMC_MOMENTS_OVERLAP): posterior-moment reductions on a side stream under the next step kernel: 0 = on (default), 1 = on, -1 = off.
   *  moments_bg_workgroups  (LMC_MOMENTS_BG_WGS): workgroups of that background reduction, 0 = by size.
   *  graph_replay: 0 or 1, no effect (the hipGraph replay it selected was removed; the field keeps the layout). */
  int32_t iterations_per_launch;
  int32_t moments_overlap;
  int32_t moments_bg_workgroups;
  int32_t graph_replay;
  /* LMC_PRIOR_EPROX */
  int32_t eprox_kind;             /* lmc_eprox_kind; LMC_PRIOR_WAVELET_L1: p, the vanishing moments of the filter (1 .. 4) */
  float eprox_p0, eprox_p1;
  int32_t eprox_scale_mask;
  /* Array-valued epsg (algs.py:509,539-542: "float or np.ndarray"; the prox parameter at algs.py:569 is then the array epsg * gamma, which the
   * closed-form proxes broadcast -- one weight per right-hand side, i.e. per chain here, or per pixel).  NULL = scalar epsg only.  Device array;
   * the prox parameter of chain c, pixel i is  epsg * gamma * prox_scale[c * prox_scale_chain_stride + i * prox_scale_pixel_stride]
   * (strides in elements: (0, 1) per pixel, (1, 0) per chain, (H*W, 1) both).  MYULA with LMC_PRIOR_L2 / L1 / EPROX only (the prox is evaluated by
   * one launch before the fused step, which consumes it); LMC_E_UNSUPPORTED for the other priors and samplers.  Must outlive the sampler. */
  /* Large PSF (see psf_kh): 0 = two 1-D passes where lmc_psf_separable accepts the kernel, 1 = require them (LMC_E_INVALID for a kernel that fails the
   * criterion), 2 = the general 2-D form always. */
  int32_t psf_separable;
  const float* prox_scale;
  int64_t prox_scale_chain_stride;
  int32_t prox_scale_pixel_stride;
  /* Box constraint x in [box_lo, box_hi] (appended; LMC_ATOMI_ABI_VERSION stays 4, struct_size tells the layouts apart).  box_enable = 0 (default): none, the
   * behaviour of before bit for bit.  1: the prior is g + the indicator of the box, and the prox is that of the sum:
   *  - LMC_PRIOR_TV_ISO / TV_ANISO: Beck and Teboulle's constrained fast gradient projection -- the primal iterate of EVERY dual iteration and the returned one
   *    are projected onto the box (not "clip afterwards": the two differ).  tv_niter >= 1 (0: LMC_E_INVALID).  Isotropic, tv_niter in {10, 20, ... 60} (after
   *    tv_lagged_output), W > 128: the full-width pipeline (myula_step_pipe_box_kernel, two teams where lmc_set_step_variant's rule for 8 holds); everything
   *    else, and the anisotropic prior at every width: the tiled kernel (myula_step_tile_box_kernel).  With a Poisson or a weighted Gaussian data term
   *    (LMC_DATA_POISSON_*, LMC_DATA_WL2_*): the box instantiations named there (tv_niter 10 on the pipeline, the tiled kernel for the rest).
   *  - LMC_PRIOR_NONE / L2 / L1 / EPROX (separable): the clamp of the prox of g, formed by one elementwise launch before the fused step (with prox_scale: the same
   *    launch).  LMC_PRIOR_NONE: the indicator alone, prox = projection.
   * Bounds: box_lo < box_hi, neither NaN (else LMC_E_INVALID); infinite ends are allowed ((0, +inf) is positivity).
   * Honoured by lmc_myula_create / lmc_sampler_step and lmc_fused_eval (the prox, and the a, t, b combination with it).  LMC_E_UNSUPPORTED, with the reason
   * in lmc_last_error: LMC_PRIOR_HAAR_L1 and LMC_PRIOR_WAVELET_L1 (not separable: clipping their prox is not the prox); tv_rtol > 0; tv_warm; lmc_mymala_create (the target would be +inf
   * outside the box); lmc_ulpda_create; lmc_skrock_create; lmc_sampler_sapg / lmc_sampler_set_prior_sigma on a handle with a box (the d / k homogeneity argument
   * does not hold on a bounded set); a forced step_variant without a box form.
   * lmc_energies, lmc_sampler_energies and lmc_prior_statistic keep reporting sigma g(x) WITHOUT the indicator: MYULA iterates live in the Moreau-Yosida
   * neighbourhood of the box, not in it. */
  int32_t box_enable;
  float box_lo, box_hi;
} lmc_problem;

/* ---- library ------------------------------------------------------------------------- */
int lmc_version(void);                 /* LMC_ATOMI_ABI_VERSION of the loaded library */
const char* lmc_last_error(void);      /* thread-local; valid until the next failing call on this thread */
int lmc_device_info(int* device, int* n_cu, size_t* lds_bytes, size_t* hbm_bytes);
/* Measured HBM streaming bandwidth of the current device: a state-shaped copy (read `bytes`, write `bytes`, 16 B per lane), the best of
 * `reps` timed passes after one warm-up over ten launch shapes, in GB/s counting both directions -- the figure bench.py prints beside the 8 TB/s spec peak
 * (SURVEY section 8(d)).  Allocates and frees 2 x bytes of HBM; synchronises `stream`. */
int lmc_hbm_copy_probe(size_t bytes, int32_t reps, float* gbs_out, void* stream);

/* ---- operator-level entry points (the prox / linear-operator plugin protocol) -------- */

/* out = H x (adjoint == 0) or H^T x (adjoint != 0) for n_img images.
 * Replaces Convolve2D.matvec / .rmatvec (prox_lmc_deconv.py:58; algs.py:284). */
int lmc_blur(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W,
             const float* h_host, int32_t kh, int32_t kw, int32_t oy, int32_t ox, int32_t adjoint, void* stream);

/* The same operator for kernels up to LMC_MAX_PSF x LMC_MAX_PSF (the operator of LMC_DATA_PSF): out = H x (adjoint == 0) or H^T x for n_img images,
 * any n_img.  separable: 0 auto, 1 require (LMC_E_INVALID where lmc_psf_separable rejects the kernel), 2 the general form.  Not in place. */
int lmc_psf_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W,
                  const float* h_host, int32_t kh, int32_t kw, int32_t oy, int32_t ox, int32_t adjoint, int32_t separable, void* stream);
/* Host only, no device needed.  1 when h (kh x kw, row-major) is an outer product u v^T to a fraction of float32 rounding, 0 when not, LMC_E_INVALID
 * for bad arguments.  With the pivot (pa, pb) of largest magnitude, u_a = h[a][pb] / h[pa][pb] and v_b = h[pa][b] formed in double must satisfy
 * |u_a v_b - h_ab| <= 2^-22 |h_ab| for every tap (so a zero tap is reproduced as zero).  u_out (kh floats) and v_out (kw floats) may be NULL; they are
 * written when the answer is 1. */
int lmc_psf_separable(const float* h_host, int32_t kh, int32_t kw, float* u_out, float* v_out);

/* The transforms of LMC_DATA_SPECTRAL, norm = "ortho", on the half plane: H and W powers of two in 8 .. 1024 (LMC_E_UNSUPPORTED otherwise), any n_img.
 * lmc_rfft2: x_dev real [n][H][W] -> out_dev complex [n][H][W / 2 + 1] (interleaved floats), numpy.fft.rfft2(x, norm="ortho").
 * lmc_irfft2: x_dev complex [n][H][W / 2 + 1] -> out_dev real [n][H][W], numpy.fft.irfft2(c, s=(H, W), norm="ortho"); x_dev is not modified.
 * lmc_spectral_filter: out = irfft2(M rfft2(x)) with the complex multiplier m_dev = [2][H][W / 2 + 1] (Re M, then Im M).  Not in place. */
int lmc_rfft2(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream);
int lmc_irfft2(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream);
int lmc_spectral_filter(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* m_dev, void* stream);
/* Host only, no device needed.  The [11][H][W / 2 + 1] float planes of LMC_DATA_SPECTRAL (what y_dev points to, once uploaded) from G and b, each
 * [H][W] complex as interleaved float64, full plane; the fold runs in float64 and every entry is rounded once. */
int lmc_spectral_tables(const double* G_host, const double* b_host, int32_t H, int32_t W, float* out_host);

/* The Radon operator of LMC_DATA_RADON (its text above is the definition): adjoint == 0 -- x_dev images [n][H][W] -> out_dev sinograms
 * [n][n_angles][n_det]; adjoint != 0 -- x_dev sinograms -> out_dev images.  angles_host: n_angles floats in radians, 1 .. LMC_MAX_RADON_ANGLES, finite;
 * n_det in 1 .. LMC_MAX_RADON_DET; any n_img.  Not in place. */
int lmc_radon_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, const float* angles_host, int32_t n_angles, int32_t n_det,
                    int32_t adjoint, void* stream);
/* Host only, no device needed.  The two tables of that definition as the kernels read them: ax_out [n_angles][W], by_out [n_angles][H] (either may be
 * NULL), float64 products rounded once. */
int lmc_radon_tables(const float* angles_host, int32_t n_angles, int32_t n_det, int32_t H, int32_t W, float* ax_out, float* by_out);

/* The operator of LMC_DATA_SENSE (its text above is the definition).  desc_dev: device floats [1 + 2 n_coils][H][W], plane 0 = M, planes 1 + 2c,
 * 2 + 2c = Re S_c, Im S_c (the head of the kind's descriptor; data planes behind it are not read).  adjoint == 0 -- in_dev real [n][H][W] -> out_dev
 * complex [n][n_coils][H][W] (interleaved floats), M . F(S_c . x); adjoint != 0 -- that shape -> out_dev real [n][H][W],
 * sum_c Re[conj(S_c) . F^H(M . k_c)]; in_dev is not modified.  H and W powers of two in 8 .. 1024 (LMC_E_UNSUPPORTED otherwise), n_coils in
 * 1 .. LMC_MAX_COILS, any n_img.  Not in place. */
int lmc_sense_apply(const float* desc_dev, const float* in_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t n_coils, int32_t adjoint,
                    void* stream);
/* Host only, no device needed.  max_k M_k^2 max_p sum_c |S_c(p)|^2 of such a descriptor on the host, in float64: L_f without sigma_f.  A negative
 * value (an lmc_status) for bad arguments. */
double lmc_sense_lipschitz(const float* desc_host, int32_t H, int32_t W, int32_t n_coils);

/* out[2][H][W] = forward-difference gradient of x (zero in last row/col); pylops.Gradient.matvec
 * (prox_lmc_deconv.py:98; algs.py:436,448). */
int lmc_gradient(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream);
/* out[H][W] = Gradient.rmatvec(y[2][H][W]) = -div (algs.py:437,443). */
int lmc_gradient_adjoint(const float* y_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, void* stream);

/* out = a*x - t*grad f(x) + b*prox_{pt * g}(x)  for n_img images, one fused launch.
 *   (a,t,b) = (0,-1,0): out = grad f(x)          -> proxf.grad        (algs.py:569; 283-284)
 *   (a,t,b) = (0, 0,1): out = prox_{pt*g}(x)     -> proxg.prox(x, pt) (algs.py:569)
 * `pt` is the prox parameter (epsg*gamma in MYULA). */
int lmc_fused_eval(const lmc_problem* prob, const float* x_dev, float* out_dev, int64_t n_img,
                   float a, float t, float b, float pt, void* stream);

/* Implicit data step  out = prox_{tau f}(x) = (I + tau*sigma_f*Op^T Op)^{-1} (x + tau*sigma_f*Op^T y)  for n_img images:
 * pyproximal.L2.prox / algs.py:224-256 (row a8).  LMC_DATA_BLUR: iterative, started from `out` as given if warm != 0, else from zero,
 * to the relative residual of lmc_set_cg_tolerance within at most `niter` iterations (the reference: LSQR, niter=50, warm start).
 * Build-specified solver: the Chebyshev semi-iteration on the known spectrum [1, 1 + tau*sigma_f*(sum|h|)^2] where the row-streaming
 * kernel covers the blur (separable, <= 7 centred taps, any width) and the tolerance is reachable within `niter` (ULPDA samplers run two
 * iterations per launch where that pays: uniform 5 x 5 box, W % 4 == 0, W <= 512, n_chains * H >= 2^17);
 * conjugate gradients otherwise (then a cap that binds returns CG's truncated iterate).
 * IDENTITY / MASK / NONE: closed form.  workspace_dev: 5*n_img*H*W floats followed (8-byte aligned) by 4*n_img+1 doubles;
 * lmc_l2_prox_workspace_bytes gives the size. */
size_t lmc_l2_prox_workspace_bytes(int64_t n_img, int32_t H, int32_t W);
int lmc_l2_prox(const lmc_problem* prob, const float* x_dev, float* out_dev, int64_t n_img, float tau, int32_t niter,
                int32_t warm, void* workspace_dev, void* stream);

/* f_out[i] = f(x_i), g_out[i] = g(x_i) (double, device, n_img each; either may be NULL).
 * Replaces proxf(x), proxg(x) of the energy log (algs.py:461-466, 578-582). */
int lmc_energies(const lmc_problem* prob, const float* x_dev, int64_t n_img,
                 double* f_out_dev, double* g_out_dev, void* stream);

/* out = prox_{thr * ||W_detail . ||_1}(x): 3-level orthonormal Haar, soft threshold of the detail coefficients.  H, W % 8 == 0. */
int lmc_haar_l1_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, float thr, void* stream);

/* The transform of LMC_PRIOR_WAVELET_L1 (its text above is the definition; p in 1 .. 4, levels in 1 .. LMC_MAX_WAVELET_LEVELS, the shape
 * preconditions there: LMC_E_INVALID otherwise).
 * lmc_wavelet_filter: host only, no device needed.  The compiled-in scaling taps h[0 .. 2p-1] in float64 into h_out (8 doubles are enough), their
 * number into *len_out (nullable).
 * lmc_wavelet_apply: out = W x (inverse == 0) or W^T x (inverse != 0) for n_img images, not in place.  Coefficients are in Mallat layout: the
 * approximation at the top-left, (H >> levels) x (W >> levels); the details of level j in the three other quadrants of the (H >> (j-1)) x (W >> (j-1))
 * corner -- rows-hi (filtered g along the rows) to the right, columns-hi below, both in the lower right.
 * lmc_wavelet_l1_prox: out = W^T S(W x), S the soft threshold thr >= 0 on every detail coefficient; not in place. */
int lmc_wavelet_filter(int32_t p, double* h_out, int32_t* len_out);
int lmc_wavelet_apply(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t p, int32_t levels, int32_t inverse, void* stream);
int lmc_wavelet_l1_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t p, int32_t levels, float thr, void* stream);

/* The prox and the value of LMC_PRIOR_VTV (its text above is the definition) on n_img multi-channel images in channel-major layout.
 * lmc_vtv_prox: out = prox_{t_sigma VTV}(x), niter dual iterations (1 .. LMC_MAX_TV_ITERS) of step `step` (0 -> 1/8) with the momentum table betas_host
 * (niter floats; NULL: the default table); box_enable != 0: the constrained form on [box_lo, box_hi] (box_lo < box_hi, neither NaN, infinite ends allowed;
 * else LMC_E_INVALID).  out has the layout of x; not in place.  t_sigma = 0 is the identity (out = x, box or not); negative or NaN: LMC_E_INVALID.
 * n_channels outside 1 .. LMC_MAX_CHANNELS, or a channel_stride below n_img * H * W with more than one channel: LMC_E_INVALID.  Work buffers (the dual
 * state of a chained prox, the partial sums of the value) come from the workspace of the stateless calls.
 * lmc_vtv_value: out_dev[n] = VTV(x_n), unweighted, n_img doubles on the device.
 * lmc_vtv_plan: host only, no device needed.  The launch plan of a prox of niter iterations on n_channels channels: the tile a workgroup owns (its patch is
 * the tile plus a halo of iters_per_launch pixels, one more on a chained prox), the dual iterations of one launch and the launches; niter <= 10 is one
 * launch at every channel count.  H and W >= 1 are checked and do not change the plan.  Every output may be NULL. */
int lmc_vtv_prox(const float* x_dev, float* out_dev, int64_t n_img, int32_t n_channels, int64_t channel_stride, int32_t H, int32_t W, float t_sigma,
                 int32_t niter, float step, const float* betas_host, int32_t box_enable, float box_lo, float box_hi, void* stream);
int lmc_vtv_value(const float* x_dev, double* out_dev, int64_t n_img, int32_t n_channels, int64_t channel_stride, int32_t H, int32_t W, void* stream);
int lmc_vtv_plan(int32_t H, int32_t W, int32_t n_channels, int32_t niter, int32_t* tile_h, int32_t* tile_w, int32_t* iters_per_launch, int32_t* n_launches);

/* The prox of LMC_PRIOR_TGV (its text above is the definition) on n_img single-plane images [n][H][W].
 * lmc_tgv_prox: out = prox_{t g}(x) with t_sigma = t sigma, niter iterations (1 .. LMC_MAX_TGV_ITERS) of step `step` (0 -> 1 / sqrt(12); 12 step^2 > 1:
 * LMC_E_INVALID); alpha0 finite and > 0; w_out_dev: NULL, or [n][2][H][W] floats that receive the auxiliary field w (row component first); box_enable
 * != 0: the constrained form on [box_lo, box_hi] (box_lo < box_hi, neither NaN, infinite ends allowed; else LMC_E_INVALID).  Not in place.  t_sigma = 0
 * is the prox of the indicator alone (out = x, or its clamp; w = 0); negative or NaN: LMC_E_INVALID.  The two 11-plane state buffers of a chained
 * prox (niter > lmc_tgv_launch_iters()) come from the workspace of the stateless calls.
 * lmc_tgv_launch_iters: host only.  The iterations one launch of tgv_prox_kernel holds; a prox of more is ceil(niter / that) chained launches. */
int lmc_tgv_prox(const float* x_dev, float* out_dev, float* w_out_dev, int64_t n_img, int32_t H, int32_t W, float t_sigma, float alpha0, int32_t niter,
                 float step, int32_t box_enable, float box_lo, float box_hi, void* stream);
int lmc_tgv_launch_iters(void);

/* Chain probes for convergence diagnostics across chains (split R-hat / effective sample size; SURVEY 8(f).3 -- absent in the
 * reference, whose only diagnostics are the per-iterate scalars of prox_lmc_deconv.py:128-133): every image is reduced to a
 * ph x pw grid of block means, out[i][a][b] = mean of x_i over rows [a*H/ph, (a+1)*H/ph) x columns [b*W/pw, (b+1)*W/pw)
 * (integer division).  1 <= ph <= H, 1 <= pw <= W, W <= 8192.  out_dev: n_img*ph*pw floats. */
int lmc_chain_probes(const float* x_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W, int32_t ph, int32_t pw, void* stream);

/* Stateless, operator level: ADDS the pixel histogram of x[C][H][W] into counts_dev [(n_bins+2)*H*W] uint64 (rows as documented at
 * lmc_sampler_set_histogram; 1 <= n_bins <= 62; lo_dev, scale_dev: [H*W] floats). */
int lmc_pixel_histogram(const float* x_dev, int64_t C, int32_t H, int32_t W, int32_t n_bins,
                        const float* lo_dev, const float* scale_dev, uint64_t* counts_dev, void* stream);

/* Stateless, operator level: ADDS the chain-group moments of x[C][H][W] into sum_dev and sumsq_dev ([n_groups*H*W] float64 each; groups and
 * arithmetic as documented at lmc_sampler_set_chain_groups; 2 <= n_groups <= LMC_MAX_CHAIN_GROUPS, chain_offset >= 0).  One owner per (group,
 * pixel) and launch, no atomics: the same call on the same arrays gives the same bits, and calls that share sum_dev / sumsq_dev must be ordered
 * (one stream). */
int lmc_group_moments(const float* x_dev, int64_t C, int64_t chain_offset, int32_t H, int32_t W, int32_t n_groups,
                      double* sum_dev, double* sumsq_dev, void* stream);

/* Stateless, operator level: ADDS the covariance sketch of x[C][H][W] (definition and arithmetic at lmc_sampler_set_cov_sketch) into y_dev
 * [k*H*W], s_dev [k] and q_dev [k*k] (float64 each).  probes_dev: [k*H*W] floats, 1 <= k <= LMC_MAX_COV_PROBES; center_dev: [H*W] floats or NULL
 * (= 0).  workspace_dev: lmc_cov_sketch_workspace_bytes(C, H, W, k) bytes of device memory, 16-byte aligned, overwritten by every call (the
 * function returns 0 for arguments the call would refuse).  One owner per output element and launch, no atomics: the same call on the same arrays
 * gives the same bits, and calls that share y / s / q or the workspace must be ordered (one stream). */
size_t lmc_cov_sketch_workspace_bytes(int64_t C, int32_t H, int32_t W, int32_t k);
int lmc_cov_sketch(const float* x_dev, int64_t C, int32_t H, int32_t W, int32_t k, const float* probes_dev, const float* center_dev,
                   double* y_dev, double* s_dev, double* q_dev, void* workspace_dev, void* stream);

/* Per-pixel projection of the stacked field y[2][H][W] onto the l2 ball (isotropic != 0) or the
 * box (isotropic == 0) of radius `radius`: L21.proxdual / L1.proxdual (algs.py:436,448). */
int lmc_dual_project(const float* y_dev, float* out_dev, int64_t n_img, int32_t H, int32_t W,
                     float radius, int32_t isotropic, void* stream);

/* Closed-form elementwise proxes of prox.py (the functional plugin surface), n elements.  Each is accurate to a few fp32 eps of its RESULT for
 * parameters 1e-5 .. 1e2 (DESIGN.md "Closed-form proxes: accuracy").  gamma, tau, omega (gamma family, uniform) and kappa are weights or bounds:
 * 0 is allowed (a weight of 0 gives the identity), a negative or NaN one is LMC_E_INVALID. */
typedef enum lmc_eprox_kind {
  LMC_EPROX_LAPLACE = 0,            /* prox.py:18  params: gamma                */
  LMC_EPROX_UNCENTERED_LAPLACE = 1, /* prox.py:22  params: gamma, mu            */
  LMC_EPROX_GAUSSIAN = 2,           /* prox.py:26  params: gamma                */
  LMC_EPROX_GEN_GAUSSIAN_4_3 = 3,   /* prox.py:31  params: gamma                */
  LMC_EPROX_GEN_GAUSSIAN_3_2 = 4,   /* prox.py:34                               */
  LMC_EPROX_GEN_GAUSSIAN_3 = 5,     /* prox.py:36                               */
  LMC_EPROX_GEN_GAUSSIAN_4 = 6,     /* prox.py:38                               */
  LMC_EPROX_HUBER = 7,              /* prox.py:44  params: gamma, tau           */
  LMC_EPROX_SMOOTHED_LAPLACE = 8,   /* prox.py:52  params: gamma                */
  LMC_EPROX_EXP = 9,                /* prox.py:56  params: gamma                */
  LMC_EPROX_GAMMA = 10,             /* prox.py:60  params: omega, kappa         */
  LMC_EPROX_CHI = 11,               /* prox.py:64  params: kappa                */
  LMC_EPROX_UNIFORM = 12,           /* prox.py:68  params: omega                */
  LMC_EPROX_TRIANGULAR = 13,        /* prox.py:78  params: omega1, omega2       */
  LMC_EPROX_LAPLACE_CONJ = 14       /* prox.py:9 applied to prox_laplace; params: gamma */
} lmc_eprox_kind;
int lmc_prox_elementwise(int32_t kind, const float* x_dev, float* out_dev, int64_t n,
                         const float* params_host, int32_t n_params, void* stream);

/* ---- MYULA sampler (replaces algs.MoreauYosidaUnadjustedLangevin, algs.py:477-587) --- */

typedef struct lmc_sampler lmc_sampler; /* opaque */

typedef struct lmc_myula_config {
  uint32_t struct_size;     /* = sizeof(lmc_myula_config) */
  lmc_problem problem;
  int32_t n_chains;         /* chains resident on this GPU */
  int64_t chain_offset;     /* global id of local chain 0 (keys the RNG; sharding-invariant noise) */
  float tau, gamma, epsg;   /* step, Moreau smoothing, scaling of g (algs.py:477-478) */
  uint64_t seed;
  int32_t noise_mode;       /* lmc_noise_mode */
  /* posterior moments: sum / sum of squares over chains and kept iterations (generalises the
   * mean over iterates at prox_lmc_deconv.py:474 to many chains, burn-in and thinning) */
  int32_t moments;          /* 0 = off */
  int32_t burn_in;          /* iterations (0-based index < burn_in) excluded */
  int32_t thin;             /* keep every thin-th iteration after burn-in (>= 1) */
} lmc_myula_config;

int lmc_myula_create(const lmc_myula_config* cfg, lmc_sampler** out);
void lmc_sampler_destroy(lmc_sampler* s);

/* MYMALA -- the Metropolis-adjusted MYULA of prox_lmc.py:134-158 at image scale, every chain at once, same configuration
 * struct.  Per iteration and chain: x' = m(x) + sqrt(2 tau) xi (the MYULA move, :150); accepted with probability
 * min(1, pi(x') q(x|x') / (pi(x) q(x'|x))), pi = exp(-f - epsg*g), q(.|b) = N(m(b), 2 tau I) (:139-143,151-154); u ~ U(0,1) from
 * Philox (ctr = (0, iteration, global chain id, 0x4C4D4302), key = seed).  A rejected chain keeps its state, which is
 * counted again by the moment accumulators (the reference's toy version drops rejected iterations from its output list).
 * All lmc_sampler_* calls apply.  LMC_E_UNSUPPORTED, with the reason in lmc_last_error: tv_warm, tv_rtol > 0, prox_scale, a Poisson data
 * term, a box constraint, and LMC_PRIOR_EPROX (a prior with a prox and no value: the target is undefined).  The weighted Gaussian data term
 * (LMC_DATA_WL2_*) is taken: it is quadratic and smooth, and f and g of the target then come from the separate energy launch.  So is the Huber data
 * term on the small operators (LMC_DATA_HUBER_IDENTITY, LMC_DATA_HUBER_BLUR: convex and C^1), in the same way. */
int lmc_mymala_create(const lmc_myula_config* cfg, lmc_sampler** out);
/* accepted_dev [n_chains] uint64: accepted proposals so far; last_log_alpha_dev [n_chains] f64 (nullable): log acceptance
 * ratio of the latest iteration.  Device buffers. */
int lmc_sampler_get_acceptance(lmc_sampler* s, uint64_t* accepted_dev, double* last_log_alpha_dev, void* stream);

/* SK-ROCK -- the stochastic orthogonal Runge-Kutta-Chebyshev scheme for the Moreau-Yosida-smoothed posterior MYULA samples (Pereyra, Vargas
 * Mieles, Zygalakis, SIAM J. Imaging Sci. 2020; Abdulle, Almuslimani, Vilmart 2018): s >= 2 evaluations of the MYULA drift per iteration, stable
 * up to delta = l_s / L with l_s = (s - 1/2)^2 (2 - 4 eta / 3) - 3/2 and L = L_f + 1/gamma, where MYULA stops near 1 / L.  Build-specified (the
 * reference has no such sampler); this text is its definition.
 *   T_j: Chebyshev polynomials of the first kind, w0 = 1 + eta / s^2, w1 = T_s(w0) / T_s'(w0)
 *   mu_1 = w1 / w0, nu_1 = s w1 / 2, kappa_1 = s w1 / w0
 *   mu_j = 2 w1 T_{j-1}(w0) / T_j(w0), nu_j = 2 w0 T_{j-1}(w0) / T_j(w0), kappa_j = -T_{j-2}(w0) / T_j(w0) = 1 - nu_j      (j = 2 .. s)
 *   drift(x) = -grad f(x) - (x - prox_{epsg gamma g}(x)) / gamma       (the drift of MYULA, algs.py:569), delta = cfg.tau, q = sqrt(2 delta)
 * One iteration draws ONE field Z ~ N(0, I):
 *   K_0 = X
 *   K_1 = X + mu_1 delta drift(X + nu_1 q Z) + kappa_1 q Z
 *   K_j = mu_j delta drift(K_{j-1}) + nu_j K_{j-1} + kappa_j K_{j-2}       (j = 2 .. s)
 *   X+  = K_s
 * For a linear drift -l x and z = -delta l this is X+ = R_s(z) X + q B_s(z) Z with R_s(z) = T_s(w0 + w1 z) / T_s(w0) and
 * B_s(z) = U_{s-1}(w0 + w1 z) / U_{s-1}(w0) (1 + w1 z / 2), U the Chebyshev polynomials of the second kind.
 *
 * lmc_skrock_coefficients: host only (no device needed).  mu, nu, kappa: n_stages doubles each, entry j - 1 = stage j; *step_factor = l_s; all
 * four nullable.  Formed in double by the three-term recurrences of T_j and T_j'.  n_stages outside 2 .. LMC_MAX_SKROCK_STAGES, or eta not finite
 * and positive: LMC_E_INVALID. */
int lmc_skrock_coefficients(int32_t n_stages, double eta, double* mu, double* nu, double* kappa, double* step_factor);
/* The sampler: lmc_myula_config as for MYULA (tau = delta), every data term, prior and non-convex term of MYULA.  Every stage is one launch of
 * the fused step kernel  a x - t grad f(x) + b prox(x) + s n  with  a = nu_j - mu_j delta / gamma, t = mu_j delta, b = mu_j delta / gamma,
 * s = kappa_j  and K_{j-2} as the injected field n; stage 1 runs on Y = X + nu_1 q Z (one streaming launch before it) with a = 1 - mu_1 delta / gamma,
 * s = (kappa_1 - nu_1) q and the same Z -- the definition up to the fp32 rounding of Y - nu_1 q Z.  One noise field per ITERATION: with
 * LMC_NOISE_PHILOX the field lmc_sampler_noise(s, iteration) returns, with LMC_NOISE_INJECTED noise_dev[iteration of the call]; the iteration
 * counter advances once per iteration.  The moment accumulators take K_s of the kept iterations (in line).  With timing enabled every stage
 * launch has its event pair: n_launches = n_stages * n_iters.  lmc_sampler_get_acceptance: LMC_E_STATE.
 * LMC_E_UNSUPPORTED for what runs outside the fused launch: tv_warm, tv_rtol > 0 on the prior, prox_scale (ncvx_rtol stays allowed).
 * n_stages / eta: as lmc_skrock_coefficients (LMC_E_INVALID). */
int lmc_skrock_create(const lmc_myula_config* cfg, int32_t n_stages, float eta, lmc_sampler** out);

/* ---- empirical-Bayes prior weight: SAPG (Vidal, De Bortoli, Pereyra, Durmus, SIAM J. Imaging Sci. 2020, Algorithm 1) ----------------------
 * The weight theta = lmc_problem.prior_sigma of a prior theta g(x), g positively homogeneous of degree k, estimated by marginal maximum
 * likelihood: one projected stochastic-gradient step on theta after every iters_per_update sampler iterations.  d/dtheta log Z(theta) =
 * -d / (k theta), so the gradient needs only g of the current samples: gbar = the mean of g(x_c) (weight 1) over the C chains of the handle.
 * Build-specified (the reference has no such estimator); this text is its definition.  With n the 0-based update index, d = dim_eff:
 *   delta_n     = step_scale (n + 1)^(-step_exponent) / d
 *   eta_{n+1}   = clamp(log(theta_n) + delta_n (d / k - theta_n gbar), log(theta_min), log(theta_max))
 *   theta_{n+1} = exp(eta_{n+1});  a clamped step returns the bound itself, bit for bit
 * (the log-parametrised form of the authors' code), all in double.
 *
 * lmc_prior_statistic: stat_dev[i] = g(x_i) with weight 1 (n_img doubles on the device): float64 sums of the fp32 per-pixel terms of
 * lmc_energies, every image summed in a fixed order (two runs give equal bits), one streaming read of x and no data term.  Stateless; only
 * struct_size, prior_kind, H and W of prob are read (LMC_PRIOR_WAVELET_L1: tv_niter and eprox_kind too, its levels and p).  LMC_PRIOR_NONE / LMC_PRIOR_EPROX (no defined value): LMC_E_UNSUPPORTED. */
int lmc_prior_statistic(const lmc_problem* prob, const float* x_dev, int64_t n_img, double* stat_dev, void* stream);

/* The weight for every later launch of this handle: after the call the handle runs exactly what a sampler created with prior_sigma = sigma
 * runs.  MYULA and SK-ROCK handles (tv_rtol > 0 included: the predicted pass counts correct themselves).  LMC_E_UNSUPPORTED: MYMALA (its
 * cached Metropolis energy would go stale), ULPDA, tv_warm (the carried dual belongs to the old weight), prox_scale, and priors without a
 * weight (LMC_PRIOR_NONE, LMC_PRIOR_EPROX).  sigma not finite or <= 0: LMC_E_INVALID. */
int lmc_sampler_set_prior_sigma(lmc_sampler* s, float sigma);

typedef struct lmc_sapg_config {
  uint32_t struct_size;                  /* = sizeof(lmc_sapg_config) */
  double theta0, theta_min, theta_max;   /* 0 < min <= theta0 <= max */
  double dim_eff;                        /* 0 = the default of lmc_sapg_dimension */
  double step_scale, step_exponent;      /* c0 > 0;  0.5 < p <= 1 */
  int32_t warmup_iters;                  /* sampler iterations at theta0 before the first update, >= 0 */
  int32_t n_updates;                     /* >= 1 */
  int32_t iters_per_update;              /* >= 1 */
  int32_t average_from;                  /* theta_bar = mean of theta_n, average_from < n <= n_updates;  0 <= average_from < n_updates */
} lmc_sapg_config;

/* Host only, no device needed.  lmc_sapg_dimension: the default d and the degree k of the prior of prob (struct_size, prior_kind, H, W are
 * read): L1 (H W, 1), L2 (H W, 2), TV_ISO / TV_ANISO (H W - 1, 1: constants are in the null space of g), HAAR_L1 (H W - (H/8)(W/8), 1: the
 * number of detail coefficients), WAVELET_L1 (H W - (H >> L)(W >> L), 1: tv_niter = L and eprox_kind = p are read too); LMC_PRIOR_NONE / LMC_PRIOR_EPROX: LMC_E_UNSUPPORTED.  Either output may be NULL.
 * lmc_sapg_update: *theta_next = theta_{n+1} of the definition above for a prior of degree k = 1, from the same inline function the update
 * kernel of lmc_sampler_sapg is compiled from (for degree k pass step_scale / k and k gbar: the same step).  cfg is checked as by
 * lmc_sampler_sapg and cfg->dim_eff must be > 0 here; n < 0, theta not finite or <= 0, gbar not finite: LMC_E_INVALID. */
int lmc_sapg_dimension(const lmc_problem* prob, double* dim_eff, double* degree);
int lmc_sapg_update(const lmc_sapg_config* cfg, int64_t n, double theta, double gbar, double* theta_next);

/* The loop on a MYULA or SK-ROCK handle: warmup_iters sampler iterations at theta0, then n_updates times { iters_per_update iterations, the
 * statistic of the new state, the update kernel (one workgroup: the float64 mean of the statistic in a fixed order, the update above, the
 * device traces, theta_{n+1} into a pinned host-mapped double), one host wait on an event recorded after that kernel, the new weight set as by
 * lmc_sampler_set_prior_sigma }.  No stream synchronisation and no copy of the state.  The iteration counter advances as in lmc_sampler_step;
 * the moment, block-moment, histogram and chain-group accumulators take nothing during the call (samples at a moving theta do not belong in them; the
 * count is unchanged).  On return the handle's weight is *theta_bar.
 * theta_trace_host: n_updates + 1 doubles, [0] = theta0; gbar_trace_host: n_updates doubles, nullable; theta_bar nullable;
 * noise_dev: [warmup_iters + n_updates * iters_per_update][C][H][W] with LMC_NOISE_INJECTED, else NULL.
 * Refusals of lmc_sampler_set_prior_sigma (LMC_E_UNSUPPORTED), then a bad cfg (LMC_E_INVALID). */
int lmc_sampler_sapg(lmc_sampler* s, const lmc_sapg_config* cfg, const float* noise_dev,
                     double* theta_trace_host, double* gbar_trace_host, double* theta_bar, void* stream);

/* x_dev: [n_chains][H][W].  x0 of algs.py:559 (copied). */
int lmc_sampler_set_state(lmc_sampler* s, const float* x_dev, void* stream);
int lmc_sampler_get_state(lmc_sampler* s, float* x_dev, void* stream);
/* Run n_iters iterations of algs.py:564-570 on every chain.  noise_dev is
 * [n_iters][n_chains][H][W] when noise_mode == LMC_NOISE_INJECTED, else NULL.
 * All work is enqueued on `stream`.  The posterior-moment reductions of all but the last iteration of a call run on an internal side stream
 * under the following step kernel (ABI 3: at every size; lmc_problem.moments_overlap = -1 / LMC_MOMENTS_OVERLAP=0 keeps them in line, and so
 * does lmc_sampler_enable_timing); the call still returns with everything it enqueued ordered before whatever the caller enqueues on
 * `stream` next. */
int lmc_sampler_step(lmc_sampler* s, int32_t n_iters, const float* noise_dev, void* stream);
/* iteration counter (number of completed iterations since creation / last set_iteration) */
int64_t lmc_sampler_iteration(const lmc_sampler* s);
int lmc_sampler_set_iteration(lmc_sampler* s, int64_t it);

/* sum_dev, sumsq_dev: [H][W] double (device).  count = samples accumulated (chains*kept its). */
int lmc_sampler_get_moments(lmc_sampler* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
int lmc_sampler_reset_moments(lmc_sampler* s, void* stream);
/* Multi-scale moments: for every enabled scale s, over the same kept samples x as the pixel moments (the same count), with
 * b(x) = the sum of x over the block [i s, min((i+1) s, H)) x [j s, min((j+1) s, W)) (edge blocks are partial), the library keeps
 * sum b and sum b^2 in float64, b itself formed in float64.  The accumulators are block SUMS: the mean and the variance of a block
 * mean follow with the block's own pixel count.  One fused reduction reads a kept iterate once for the pixels and all scales;
 * with no scale enabled the library launches exactly what it launches without this call.
 * scales: n_scales distinct values out of {2,4,8,16}; n_scales = 0 turns them off.  Needs cfg.moments != 0 (else LMC_E_STATE) and
 * count == 0, i.e. right after create or lmc_sampler_reset_moments (else LMC_E_STATE).  Anything else in scales: LMC_E_INVALID. */
int lmc_sampler_set_moment_scales(lmc_sampler* s, int32_t n_scales, const int32_t* scales);
/* sum_dev, sumsq_dev: [ceil(H/scale)][ceil(W/scale)] double (device, either nullable).  A scale that is not enabled: LMC_E_INVALID. */
int lmc_sampler_get_block_moments(lmc_sampler* s, int32_t scale, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
/* Pixel histograms: over the same kept samples as the pixel moments (the same count) the library keeps, per pixel p, n_bins + 2
 * unsigned 64-bit counters.  A sample v (fp32) is classified in fp32 by t = (v - lo[p]) * scale[p] -- one subtraction, then one
 * multiplication; scale is bins per unit, n_bins / (hi - lo) -- into row 0 (t < 0), row 1 + floor(t) (0 <= t < n_bins) or row
 * n_bins + 1 (everything else: t >= n_bins, +inf, NaN), so the rows of a pixel always sum to count.  Integer atomics: the counts do
 * not depend on launch shapes or orders.  The histogram is a launch of its own after the moment reduction of the same iterate; a
 * sampler without one launches exactly what it launches without this call.
 * n_bins = 0 turns it off.  Copies lo / scale ([H*W] floats, device) into the handle.  Needs cfg.moments != 0 and count == 0
 * (else LMC_E_STATE); n_bins outside 0 .. 62 or a NULL array with n_bins > 0: LMC_E_INVALID.  lmc_sampler_reset_moments zeroes
 * the counts too. */
int lmc_sampler_set_histogram(lmc_sampler* s, int32_t n_bins, const float* lo_dev, const float* scale_dev);
/* counts_dev: [(n_bins+2)*H*W] uint64 (device, nullable).  A handle without a histogram: LMC_E_INVALID. */
int lmc_sampler_get_histogram(lmc_sampler* s, uint64_t* counts_dev, uint64_t* count, void* stream);
/* Chain-group moments: Monte-Carlo error of the pixel moments from the scatter of chain groups.  Chain c of the handle has global id
 * chain_offset + c; its group is that id mod G, so every sharding of the chains over GPUs gives every rank all groups.  Over the same kept
 * samples as the pixel moments the library keeps, in float64, A[g][p] = sum x and B[g][p] = sum x^2 per group g and pixel p ([G][H][W] each);
 * the fp32 sample is widened first, so x^2 is exact in float64.  n[g] = (kept iterations) x (chains of the handle in group g), computed on the
 * host; a group without a local chain has n = 0 and its accumulators stay zero.
 * With N = sum n, m_g = A_g / n_g, v_g = B_g / n_g - m_g^2, m = sum A_g / N, v = sum B_g / N - m^2 (float64, per pixel), the summaries are
 *   mcse_mean = sqrt(s / N),   s  = sum_g n_g (m_g - m)^2 / (G - 1)
 *   mcse_var  = sqrt(sv / N),  sv = sum_g n_g (v_g - vbar)^2 / (G - 1),  vbar = sum n_g v_g / N
 *   ess       = N v / s        (+inf where s = 0, not a clamp)
 * For equal n_g this is the textbook standard error of G independent replicate means -- it includes the autocorrelation of the chains and needs
 * neither lags nor a stored iterate; the weights keep it unbiased when the chain count is no multiple of G.  The relative precision of s is
 * sqrt(2 / (G - 1)): about 25 % at G = 32 and 18 % at G = 64, which is why the cap is 64 and not 8.  The library keeps the accumulators; the
 * summaries are host arithmetic on them (mcse_from_group_moments in the Python package).
 * The pass is a launch of its own after the moment reduction (and the histogram) of the same iterate, one owner per (group, pixel) and no
 * atomics: equal runs give equal bits.  A sampler without groups launches exactly what it launches without this call.  lmc_sampler_sapg
 * suspends these accumulators with the others.
 * n_groups = 0 turns them off; n_groups may exceed the handle's chain count (empty groups).  Needs cfg.moments != 0 and count == 0 (else
 * LMC_E_STATE); n_groups outside {0, 2 .. LMC_MAX_CHAIN_GROUPS}: LMC_E_INVALID.  lmc_sampler_reset_moments zeroes the accumulators too. */
int lmc_sampler_set_chain_groups(lmc_sampler* s, int32_t n_groups);
/* sum_dev, sumsq_dev: [n_groups*H*W] double (device, nullable); counts_host: [n_groups] (host, nullable).  A handle without groups:
 * LMC_E_INVALID. */
int lmc_sampler_get_group_moments(lmc_sampler* s, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream);
/* Covariance sketch: how pixels move together, without a stored iterate.  Given k probe images P[k][H][W] (fp32, 1 <= k <= LMC_MAX_COV_PROBES) and a
 * centre m[H][W] (fp32, NULL = 0), every kept sample x_c (chain c) contributes
 *   d_c[p]  = x_c[p] - m[p]                      (one fp32 subtraction)
 *   t_c[j]  = sum_p P[j][p] d_c[p]               (the projection of the sample on probe j)
 *   Y[j][p] += sum_c t_c[j] d_c[p]               [k][H][W] float64
 *   s[j]    += sum_c t_c[j]                      [k]       float64
 *   Q[j][l] += sum_c t_c[j] t_c[l]               [k][k]    float64
 * over the same kept samples, and with the same count, as the pixel moments s1, s2.  With n = count, dbar = s1 / n - m and tbar = s / n (float64
 * host arithmetic; cov_from_sketch in the Python package) the summaries are
 *   cov_xt[j][p] = Y[j][p] / n - tbar[j] dbar[p]     = (Sigma P_j^T)[p], Sigma the N x N posterior sample covariance: every pixel against projection j
 *   cov_tt       = Q / n - tbar tbar^T               = P Sigma P^T, k x k
 * exactly.  Region indicators as probes give the covariance matrix of the region fluxes and the correlation map of every pixel with a region;
 * Gaussian random probes give the one-pass Nystrom sketch Sigma ~ cov_xt^T cov_tt^+ cov_xt of the leading uncertainty modes (exact when
 * rank Sigma <= k; it underestimates eigenvalues otherwise).  Without a centre cov_xt is a difference of terms of size mean^2 and loses digits:
 * pass a pilot-run mean as centre.
 * Arithmetic: t_c[j] is formed from fp32 products accumulated in fp32 (an ordered fmaf chain) over runs of at most 2048 pixels, the run sums are
 * combined in float64 in ascending order.  In the Y update t is rounded to fp32, the products are accumulated in fp32 over runs of at most 1024
 * chains, and the run sums are added to Y in float64 with a plain read-add-write.  s and Q are float64 sums of the float64 t.  No float atomics,
 * one owner per output element and launch: equal runs give equal bits.  Tails are zero-filled operands.
 * The passes are launches of their own after the moment reduction (the histogram, the chain-group moments) of the same iterate; a sampler without a
 * sketch launches exactly what it launches without this call.  lmc_sampler_sapg suspends these accumulators with the others.
 * The call copies probes and centre into the handle.  k = 0 turns the sketch off.  Needs cfg.moments != 0 and count == 0 (else LMC_E_STATE); k outside
 * 0 .. LMC_MAX_COV_PROBES or NULL probes with k > 0: LMC_E_INVALID.  lmc_sampler_reset_moments zeroes Y, s and Q too. */
int lmc_sampler_set_cov_sketch(lmc_sampler* s, int32_t k, const float* probes_dev, const float* center_dev);
/* y_dev: [k*H*W], s_dev: [k], q_dev: [k*k] double (device, nullable); count: kept samples.  A handle without a sketch: LMC_E_INVALID. */
int lmc_sampler_get_cov_sketch(lmc_sampler* s, double* y_dev, double* s_dev, double* q_dev, uint64_t* count, void* stream);
/* per-chain energies f(x_c), g(x_c) of the current state (device double [n_chains]) */
int lmc_sampler_energies(lmc_sampler* s, double* f_out_dev, double* g_out_dev, void* stream);
/* the noise field xi[n_chains][H][W] the sampler draws at `iteration` (parity rung R3) */
int lmc_sampler_noise(lmc_sampler* s, int64_t iteration, float* out_dev, void* stream);
/* HIP-event timing of the step kernels: when enabled, lmc_sampler_step brackets EACH step-kernel
 * launch with its own event pair on the launch stream (interleaved moment reductions stay outside, and run in line -- not on the side
 * stream -- so that the step kernel is timed alone).
 * last_step_timing returns the summed kernel milliseconds and the number of launches of the LAST
 * lmc_sampler_step call (bench.py's roofline leg); it synchronises on the last event. */
int lmc_sampler_enable_timing(lmc_sampler* s, int32_t on);
int lmc_sampler_last_step_timing(lmc_sampler* s, float* total_ms, int32_t* n_launches);
/* name of the step kernel variant selected for this configuration (for profiles/) */
const char* lmc_sampler_kernel_name(const lmc_sampler* s);
/* Early-exit statistics of the latest TV prox evaluated with tv_rtol > 0 (which = 0) or of the ME-TV inner prox with ncvx_rtol > 0 (which = 1)
 * on the device path: passes_dev [n_chains] int32 (device, nullable) = the loop pass each chain left in (tv_niter: it ran out of passes);
 * reruns_host[4] (host, nullable) = chains whose run had to be repeated after round 1 / 2 / 3 / 4, summed over all calls since creation
 * (round 4's count stays 0 by construction).  Synchronises `stream`.  LMC_E_STATE when the sampler does not use the device path. */
int lmc_sampler_tv_exit_stats(lmc_sampler* s, int32_t which, int32_t* passes_dev, uint64_t* reruns_host, void* stream);

/* ---- multi-channel MYULA sampler: colour, Bayer mosaics, dual-energy pairs under the vectorial TV prior --------------------------------
 * A handle type of its own (lmc_mch.hip), not an lmc_sampler: that type's pair launches, early exits, warm duals and side-stream moments stay as they
 * are.  The posterior is exp(-sum_ch f_ch(x_ch) - epsg sigma VTV(x)); one iteration is MYULA's (lmc_myula_create) on all channels at once, in two stages:
 *   prox   lmc_vtv_prox at the parameter epsg gamma sigma over all chains and channels, into a buffer of the handle;
 *   step   per channel ONE launch of the fused step kernel of the same problem without a prior, which consumes that channel's block of the buffer as a
 *          ready-made prox: x_ch <- (1 - tau / gamma) x_ch - tau grad f_ch(x_ch) + (tau / gamma) prox_ch + sqrt(2 tau) xi_ch.
 * problem: prior_kind must be LMC_PRIOR_VTV; prior_sigma, tv_niter, tv_step, tv_betas_host and box_* are read as for LMC_PRIOR_TV_ISO; data_kind is
 * LMC_DATA_NONE, IDENTITY, BLUR or MASK; y_dev is [n_channels][H][W]; mask_dev is [H][W] (mask_channel_stride = 0: one mask for all channels) or
 * [n_channels][H][W] (mask_channel_stride = H * W: one per channel, a Bayer mosaic); sigma_f and the taps are shared by the channels.
 * State and injected noise are [n_channels][n_chains][H][W] ([n_iters] in front for the noise): channel-major, each channel's chains contiguous.
 * Noise: channel ch draws the Philox field of the seed (seed + (ch << 32)) mod 2^64 -- key1 = (uint32)(seed >> 32) + ch -- so channel 0 is the field of
 * a grey sampler of the same seed, and any sharding of the chains (chain_offset) reproduces the same trajectories.
 * Moments: [n_channels][H][W] doubles for the sum and the sum of squares (the reductions of lmc_sampler_get_moments, one accumulator per channel) and one
 * count = kept iterates x chains.  Energies: f[c] = sum_ch f_ch(x_ch,c) (the energy launches of lmc_sampler_energies per channel, added in float64),
 * g[c] = sigma VTV(x_c) (without the indicator of a box, as everywhere).
 * LMC_E_UNSUPPORTED, with the reason in lmc_last_error: every other data_kind, ncvx_kind != LMC_NCVX_NONE, tv_rtol > 0, tv_warm, prox_scale,
 * tv_lagged_output.  LMC_E_INVALID: n_channels outside 1 .. LMC_MAX_CHANNELS, tv_niter outside 1 .. LMC_MAX_TV_ITERS, bad bounds, a
 * mask_channel_stride other than 0 or H * W, a prior_kind other than LMC_PRIOR_VTV.  Calls on one handle must be serialised by the caller. */
typedef struct lmc_mch lmc_mch; /* opaque */

typedef struct lmc_mch_config {
  uint32_t struct_size;     /* = sizeof(lmc_mch_config) */
  lmc_problem problem;
  int32_t n_channels;
  int64_t mask_channel_stride;          /* 0: one mask for all channels; H*W: one per channel (a Bayer mosaic) */
  int32_t n_chains; int64_t chain_offset; float tau, gamma, epsg; uint64_t seed; int32_t noise_mode;
  int32_t moments, burn_in, thin;
} lmc_mch_config;

int lmc_mch_create(const lmc_mch_config* cfg, lmc_mch** out);
void lmc_mch_destroy(lmc_mch* s);
int lmc_mch_set_state(lmc_mch* s, const float* x_dev, void* stream);
int lmc_mch_get_state(lmc_mch* s, float* x_dev, void* stream);
int lmc_mch_step(lmc_mch* s, int32_t n_iters, const float* noise_dev, void* stream);
int64_t lmc_mch_iteration(const lmc_mch* s);
int lmc_mch_set_iteration(lmc_mch* s, int64_t it);
int lmc_mch_get_moments(lmc_mch* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
int lmc_mch_reset_moments(lmc_mch* s, void* stream);
int lmc_mch_energies(lmc_mch* s, double* f_out_dev, double* g_out_dev, void* stream);
int lmc_mch_noise(lmc_mch* s, int64_t iteration, float* out_dev, void* stream);
/* the kernels of the latest iteration: the prox kernel and the step kernel of the last channel */
const char* lmc_mch_kernel_name(const lmc_mch* s);

/* ---- split Gibbs sampler (SGS): exact Gaussian x-step, MYULA z-step ----------------------------------------------------------------
 * Vono, Dobigeon, Chainais (2019); Pereyra, Vargas-Mieles, Zygalakis (2022).  A handle type of its own (lmc_sgs.hip) that composes existing launches.
 * Build-specified; this text is its definition.  Augmented target with the coupling parameter rho > 0:
 *   pi_rho(x, z)  ~  exp( -f(x) - epsg g(z) - ||x - z||^2 / (2 rho^2) ).
 * Its x-marginal is the posterior with g replaced by a rho^2-smoothed version of it (rho -> 0 recovers the posterior).  This is a bias of the MODEL,
 * chosen with rho; it is separate from, and adds to, the bias of the MYULA discretisation of the z-step (chosen with tau and gamma).
 * State: [2][n_chains][H][W], plane 0 = x, plane 1 = z.  With rinv = 1 / rho^2 (float32: 1 / (rho * rho)), iteration k is
 *  1. x | z, exact:  x ~ N(Q^-1 (z rinv + grad-free part of -grad f), Q^-1),  Q = Hess f + rinv I.
 *     LMC_DATA_SPECTRAL, with the half-plane tables A (real), B (complex) of lmc_spectral_tables and transforms of norm "ortho":
 *         q_k = sigma_f A_k + rinv,    x = irfft2( ( rfft2(z) rinv + sigma_f B + sqrt(q) .* rfft2(xi_x) ) / q ).
 *       xi_x is a real N(0, 1) field in pixel space: its unitary transform is the Hermitian white field, and A_k = A_-k, so x is real.
 *       Launches: fft_rows_fwd_kernel on z and on xi_x, ONE sgs_cols_gibbs_kernel per strip (the column transform of the noise strip is
 *       kept in registers scaled by sqrt(q), then the strip of z is transformed, the functor applied, and transformed back), fft_rows_inv_kernel.
 *     LMC_DATA_IDENTITY, LMC_DATA_MASK (mask m), LMC_DATA_WL2_IDENTITY (weights w); w = 1, m = 1 where absent; y = b:
 *         q_p = sigma_f w_p m_p^2 + rinv,    x_p = ( z_p rinv + sigma_f w_p m_p b_p + sqrt(q_p) xi_x,p ) / q_p.
 *     LMC_DATA_NONE: q = rinv.   (One elementwise kernel, sgs_xdiag_*; sqrt and the division are IEEE.)
 *     With xi_x = 0 the draw is the conditional mean, prox_{rho^2 f}(z) (what lmc_l2_prox evaluates at tau = rho^2).
 *  2. z | x, n_inner MYULA steps on exp(-epsg g(z) - ||z - x||^2 / (2 rho^2)) with step tau and smoothing gamma:
 *         z+ = z - (tau rinv)(z - x) - (tau / gamma)(z - prox_{epsg gamma g}(z)) + sqrt(2 tau) xi_z.
 *     Launches: the step kernel of the same problem with LMC_DATA_NONE -- z' = (1 - tau / gamma) z + (tau / gamma) prox + sqrt(2 tau) xi_z, every prior and
 *     box that launch takes -- then sgs_couple_kernel: z+ = fma(-(tau rinv), z_old - x, z') (the difference first, then one fma).
 *     The smooth part of the z-potential has the Lipschitz constant rinv + 1 / gamma: tau <= 1 / (rinv + 1 / gamma) is the recommended range.
 *  3. The kept iterate is x after stage 1; burn_in, thin, the pixel moments and the chain-group moments are those of lmc_sampler_* on x.
 * Noise: plane p (0: xi_x, 1: xi_z) draws the Philox field of the seed (seed + (p << 32)) mod 2^64 -- key1 = (uint32)(seed >> 32) + p -- the convention of
 * lmc_mch_*; any sharding of the chains (chain_offset) reproduces the same trajectories.  xi_x of iteration k is the field of counter k; xi_z of inner step
 * j is the field of counter k n_inner + j ((iteration + 1) n_inner must fit 32 bits).  Injected noise: [n_iters][1 + n_inner][n_chains][H][W], xi_x first.
 * lmc_sgs_noise: plane_and_inner = 0 is xi_x of `iteration`, 1 + j is xi_z of its inner step j.
 * lmc_sgs_energies: f_out[c] = f(x_c), g_out[c] = g(z_c) (0 for a prior without a value: closed-form proxes, TGV), coupling_out[c] =
 * ||x_c - z_c||^2 / (2 rho^2) (differences and squares in float64, summed in a fixed order); each may be NULL.
 * LMC_E_UNSUPPORTED, with the reason in lmc_last_error: a data term whose Hessian is diagonal in neither basis (LMC_DATA_BLUR, the large PSF, the Radon
 * operator; a periodic blur is LMC_DATA_SPECTRAL), Poisson and Huber terms (the conditional is not Gaussian), ncvx_kind != NONE, tv_rtol > 0, tv_warm,
 * prox_scale, LMC_PRIOR_VTV.  LMC_E_INVALID: rho, tau or gamma not finite and > 0, n_inner outside 1 .. LMC_MAX_SGS_INNER, spectral sides that are not
 * powers of two in 8 .. 1024.  Calls on one handle must be serialised by the caller. */
#define LMC_MAX_SGS_INNER 16
typedef struct lmc_sgs lmc_sgs; /* opaque */

typedef struct lmc_sgs_config {
  uint32_t struct_size;     /* = sizeof(lmc_sgs_config) */
  lmc_problem problem;
  int32_t n_chains; int64_t chain_offset;
  float rho, tau, gamma, epsg;
  int32_t n_inner;
  uint64_t seed; int32_t noise_mode;
  int32_t moments, burn_in, thin;
} lmc_sgs_config;

int lmc_sgs_create(const lmc_sgs_config* cfg, lmc_sgs** out);
void lmc_sgs_destroy(lmc_sgs* s);
/* x_dev: [2][n_chains][H][W], x then z */
int lmc_sgs_set_state(lmc_sgs* s, const float* x_dev, void* stream);
int lmc_sgs_get_state(lmc_sgs* s, float* x_dev, void* stream);
int lmc_sgs_step(lmc_sgs* s, int32_t n_iters, const float* noise_dev, void* stream);
int64_t lmc_sgs_iteration(const lmc_sgs* s);
int lmc_sgs_set_iteration(lmc_sgs* s, int64_t it);
int lmc_sgs_get_moments(lmc_sgs* s, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
int lmc_sgs_reset_moments(lmc_sgs* s, void* stream);
/* as lmc_sampler_set_chain_groups / lmc_sampler_get_group_moments, on the kept x */
int lmc_sgs_set_chain_groups(lmc_sgs* s, int32_t n_groups);
int lmc_sgs_get_group_moments(lmc_sgs* s, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream);
int lmc_sgs_energies(lmc_sgs* s, double* f_out_dev, double* g_out_dev, double* coupling_out_dev, void* stream);
int lmc_sgs_noise(lmc_sgs* s, int64_t iteration, int32_t plane_and_inner, float* out_dev, void* stream);
/* the kernels of the latest iteration: the x-draw, then the step kernel of the z-step */
const char* lmc_sgs_kernel_name(const lmc_sgs* s);
/* The stateless x-draw of stage 1: out = the draw of x | z for n_img images z with the white field noise_dev ([n_img][H][W]); noise_dev = NULL: the
 * conditional mean.  The prior fields of prob are validated and not used.  out_dev may not alias z_dev or noise_dev. */
int lmc_sgs_xstep(const lmc_problem* prob, const float* z_dev, const float* noise_dev, float* out_dev, int64_t n_img, float rho, void* stream);

/* ---- multi-GPU: the one collective of the path ----------------------------------------------
 * Chains are sharded over GPUs by global chain id (chain_offset), one process per GPU, no data-path collective.  The only
 * exchange is the sum of the posterior-moment accumulators over the ranks -- what generalises the `.mean(axis=0)` over iterates
 * of prox_lmc_deconv.py:474 to a multi-GPU job.
 *
 * lmc_allreduce_moments: packs this sampler's {sum x [H][W], sum x^2 [H][W], count} into one float64 buffer, runs ONE
 * ncclAllReduce(ncclSum) (RCCL over xGMI) on `stream`, writes the job-wide sums to sum_dev / sumsq_dev (device, [H][W] double,
 * nullable), synchronises `stream` and returns the job-wide count.  The sampler's own accumulators are left untouched.
 * rccl_comm: an ncclComm_t passed as void* -- from lmc_rccl_comm_create below or any communicator the host already has (e.g.
 * torch.distributed's ProcessGroupNCCL) -- with one rank per sampler; NULL = a job of one rank (plain copy).
 * librccl is dlopen'd on first use (LMC_RCCL_LIB overrides the search: librccl.so.1 already in the process, then the default
 * paths); without it these calls return LMC_E_UNSUPPORTED and everything else works. */
#define LMC_RCCL_UNIQUE_ID_BYTES 128
int lmc_rccl_available(void);
/* ncclGetUniqueId on one rank; the host distributes the 128 bytes to the others (MPI, a file, torch.distributed ...). */
int lmc_rccl_unique_id(void* id128_host);
/* ncclCommInitRank on the CURRENT device (one process per GPU).  Collective: every rank of the job calls it. */
int lmc_rccl_comm_create(void** comm_out, int32_t world, int32_t rank, const void* id128_host);
int lmc_rccl_comm_destroy(void* comm);
int lmc_allreduce_moments(lmc_sampler* s, void* rccl_comm, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
/* as lmc_allreduce_moments, for ONE scale; rccl_comm NULL = a job of one rank (plain copy).  Packs through the same code as the pixel collective. */
int lmc_allreduce_block_moments(lmc_sampler* s, void* rccl_comm, int32_t scale, double* sum_dev, double* sumsq_dev, uint64_t* count, void* stream);
/* one ncclAllReduce(ncclUint64, sum) of counts + count; rccl_comm NULL = a job of one rank (plain copy).  A handle without a histogram: LMC_E_INVALID. */
int lmc_allreduce_histogram(lmc_sampler* s, void* rccl_comm, uint64_t* counts_dev, uint64_t* count, void* stream);
/* one ncclAllReduce(ncclFloat64, sum) of the packed {A, B, n} (the counts travel as doubles, exact far below 2^53); rccl_comm NULL = a job of one
 * rank (plain copy).  A handle without groups: LMC_E_INVALID. */
int lmc_allreduce_group_moments(lmc_sampler* s, void* rccl_comm, double* sum_dev, double* sumsq_dev, uint64_t* counts_host, void* stream);

/* ---- ULPDA sampler (replaces algs.UnadjustedLangevinPrimalDual, algs.py:295-474) --------------------
 *   x    <- prox_{tau f}(x - tau (A^T y + z)) + sqrt(2 tau) xi      (algs.py:440/446)
 *   xhat <- x + theta (x - x_old)                                   (:441/447)
 *   y    <- prox_{mu g*}(y + mu A xhat)                             (:436/448)   order set by gfirst (:435)
 * A = forward-difference gradient (prox_lmc_deconv.py:98); g = problem.prior (TV_ISO -> L21, TV_ANISO -> L1);
 * f = problem data term; for LMC_DATA_BLUR the implicit step (I + tau*sigma_f*H^T H)^{-1} is solved per chain, warm-started, to the
 * tolerance of lmc_set_cg_tolerance within at most `cg_niter` iterations (Chebyshev semi-iteration or CG, see lmc_l2_prox; the
 * reference: <= 50 LSQR iterations, algs.py:247-256).
 * The handle is an lmc_sampler: set_state / get_state / step / energies / moments / noise / destroy apply. */
typedef struct lmc_ulpda_config {
  uint32_t struct_size;     /* = sizeof(lmc_ulpda_config) */
  lmc_problem problem;
  int32_t n_chains;
  int64_t chain_offset;
  float tau, mu, theta;     /* algs.py:295-296 (scalars; per-iteration arrays: lmc_sampler_set_steps between calls) */
  int32_t gfirst;           /* algs.py:296, 435 */
  int32_t cg_niter;         /* inner iterations of the implicit data step (niter=50 at prox_lmc_deconv.py:101) */
  int32_t warm;             /* warm-start the inner solver from the previous solve (warm=True at :101) */
  const float* z_dev;       /* optional additional vector z [H][W] (algs.py:438-439), NULL = none */
  uint64_t seed;
  int32_t noise_mode;
  int32_t moments, burn_in, thin;
} lmc_ulpda_config;

int lmc_ulpda_create(const lmc_ulpda_config* cfg, lmc_sampler** out);
/* dual variable y [n_chains][2][H][W] (y0 of algs.py:427; y_samples of :451) */
int lmc_sampler_set_dual(lmc_sampler* s, const float* y_dev, void* stream);
int lmc_sampler_get_dual(lmc_sampler* s, float* y_dev, void* stream);
/* change (tau, mu) for the following iterations (the reference accepts per-iteration arrays, algs.py:402-408) */
int lmc_sampler_set_steps(lmc_sampler* s, float tau, float mu);

/* Library-wide DEFAULT (used when lmc_problem.implicit_tol is 0; per-handle / per-call value: lmc_problem.implicit_tol) of the
 * relative residual |r| <= tol |b| at which the inner solver of the implicit data step (lmc_l2_prox, ULPDA) stops before
 * cg_niter / niter iterations -- the stopping rule of the reference's solver (scipy lsqr's btol, default 1e-6, at algs.py:250).
 * Decided on the device for the whole batch of chains (all must satisfy it); tol = 0 disables it (always CG, all iterations).
 * Default 1e-6.  Returns the previous value; a negative argument only queries. */
float lmc_set_cg_tolerance(float tol);

/* Library-wide DEFAULT of the step-kernel variant, used by launches whose lmc_problem.step_variant is 0 (per-handle / per-call
 * selection: lmc_problem.step_variant; this switch is process-global and not thread-safe -- A/B tests only): 0 = auto (default),
 * 1 = LDS-tiled, 2 = (removed in ABI 2: the one-group streaming pipeline; LMC_E_INVALID), 3 = the row pipeline split over two wave groups,
 * 4 = HBM-bound tiled kernel for closed-form priors, 5 = register-block kernel (stencil-free data term, prox local to
 * 8 x 8 blocks: Haar-l1 / l2 / l1 / none; H, W multiples of 8), 6 = barrier-free row streaming (separable blur + closed-form
 * prior; any width: column strips above 512 columns, dword-aligned 16-byte accesses when W % 4 != 0), 7 = stage-parallel full-width TV pipeline
 * (isotropic TV with 10, 20, ... 60 dual iterations, separable blur or no data term, W > 128; any width for these counts, other counts -- 2, 6, 8, 9,
 * warm-dual 1, 2, 3 -- need W % 4 == 0 up to 256 columns and W % 8 == 0 above), in its one-team layout (8 waves of up to 8 pixels per lane),
 * 8 = the same pipeline in its two-team layout (16 waves of 4 pixels per lane, each team on half the width; one launch of 10 dual iterations,
 * 5 x 5 blur, 264 <= W <= 512 with W % 8 == 0, no energy by-products or non-convex term; other configurations: LMC_E_UNSUPPORTED; bit-identical
 * to 7).  Auto picks the two-team layout where it covers the configuration (the headline one) and the one-team layout elsewhere.
 * LMC_PRIOR_TV_ANISO has forms of 1, 7 (tv_niter in {10, 20, ... 60}, W > 128) and 8 (the configurations named above) only, auto picks among
 * them; every other value returns LMC_E_UNSUPPORTED from the call that would launch it.  The value 8
 * is accepted since this ABI revision (additive).  Returns the previous setting (>= 0) or a negative lmc_status.  All variants compute the same update; the
 * switch exists for A/B tests and profiles. */
int lmc_set_step_variant(int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* LMC_ATOMI_H */
