"""ctypes binding of liblmc_atomi.so (include/lmc_atomi.h).

This is the only place the package touches native code.  There is NO fallback: if the
library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblmc_atomi.so")
ABI_VERSION = 4

# enums (include/lmc_atomi.h)
DATA_NONE, DATA_IDENTITY, DATA_BLUR, DATA_MASK = 0, 1, 2, 3
DATA_POISSON_IDENTITY, DATA_POISSON_BLUR, DATA_POISSON_MASK = 4, 5, 6      # y_dev: [2][H][W], the counts then the background
POISSON_KINDS = (DATA_POISSON_IDENTITY, DATA_POISSON_BLUR, DATA_POISSON_MASK)
DATA_WL2_IDENTITY, DATA_WL2_BLUR = 7, 8      # y_dev: [2][H][W], the observation then the per-pixel weights
DATA_PSF, DATA_POISSON_PSF, DATA_WL2_PSF = 9, 10, 11      # the large PSF (psf_* fields): Gaussian, Poisson, weighted Gaussian term
DATA_HUBER_IDENTITY, DATA_HUBER_BLUR, DATA_HUBER_PSF = 13, 14, 15      # the Huber data term; y_dev: [2][H][W], the observation then the thresholds delta
HUBER_KINDS = (DATA_HUBER_IDENTITY, DATA_HUBER_BLUR, DATA_HUBER_PSF)
PSF_KINDS = (DATA_PSF, DATA_POISSON_PSF, DATA_WL2_PSF, DATA_HUBER_PSF)
WL2_KINDS = (DATA_WL2_IDENTITY, DATA_WL2_BLUR)
DATA_SPECTRAL = 12      # the Fourier-domain data term: y_dev is [11][H][W / 2 + 1], the planes of lmc_spectral_tables
SPECTRAL_PLANES = 11
FFT_MIN, FFT_MAX = 8, 1024      # sides of the transforms: powers of two in this range
# the parallel-beam Radon operator (kh = n_angles, kw = n_det, h_host = the angles): Gaussian, Poisson, weighted Gaussian, Huber term; y_dev is
# sinogram-shaped, [n_angles][n_det], or [2][n_angles][n_det] for the last three
DATA_RADON, DATA_POISSON_RADON, DATA_WL2_RADON, DATA_HUBER_RADON = 16, 17, 18, 19
RADON_KINDS = (DATA_RADON, DATA_POISSON_RADON, DATA_WL2_RADON, DATA_HUBER_RADON)
MAX_RADON_ANGLES, MAX_RADON_DET, MAX_RADON_SIDE = 1024, 4096, 1 << 20
# the multi-coil SENSE term (kh = n_coils): y_dev is [1 + 4 n_coils][H][W], M, then Re / Im of every map, then Re / Im of every coil's data
DATA_SENSE = 20
MAX_COILS = 32
TWO_PLANE_KINDS = POISSON_KINDS + WL2_KINDS + (DATA_POISSON_PSF, DATA_WL2_PSF) + HUBER_KINDS      # y_dev is [2][H][W]
PRIOR_NONE, PRIOR_L2, PRIOR_L1, PRIOR_TV_ISO, PRIOR_TV_ANISO, PRIOR_HAAR_L1, PRIOR_EPROX = 0, 1, 2, 3, 4, 5, 6
PRIOR_WAVELET_L1 = 7      # Daubechies wavelet-l1: lmc_problem.tv_niter = levels, eprox_kind = p (the struct has no hole left)
PRIOR_VTV = 8             # vectorial TV of a multi-channel image: lmc_mch_* and lmc_vtv_* only, every other entry point refuses it
MAX_CHANNELS = 4
PRIOR_TGV = 9             # second-order TGV: lmc_problem.tv_niter = iterations of the prox, eprox_p0 = alpha0, tv_step = the primal-dual step (0: 1 / sqrt(12))
MAX_TGV_ITERS = 256
NOISE_PHILOX, NOISE_INJECTED, NOISE_NONE = 0, 1, 2
NCVX_NONE, NCVX_MC_TV, NCVX_ME_TV, NCVX_MC_TV_ANISO, NCVX_ME_TV_ANISO = 0, 1, 2, 3, 4
MAX_BLUR = 9
MAX_PSF = 33
MAX_TV_ITERS = 64
MAX_SKROCK_STAGES = 64
MAX_CHAIN_GROUPS = 64
MAX_COV_PROBES = 32
MAX_WAVELET_LEVELS = 8
WAVELETS = {"haar": 1, "db1": 1, "db2": 2, "db3": 3, "db4": 4}      # name -> p, the vanishing moments of the filter
(EPROX_LAPLACE, EPROX_UNCENTERED_LAPLACE, EPROX_GAUSSIAN, EPROX_GEN_GAUSSIAN_4_3, EPROX_GEN_GAUSSIAN_3_2,
 EPROX_GEN_GAUSSIAN_3, EPROX_GEN_GAUSSIAN_4, EPROX_HUBER, EPROX_SMOOTHED_LAPLACE, EPROX_EXP, EPROX_GAMMA,
 EPROX_CHI, EPROX_UNIFORM, EPROX_TRIANGULAR, EPROX_LAPLACE_CONJ) = range(15)
# lmc_eprox_kind -> (name, parameter names in the order of prox.py, indices of the parameters that are weights, scales or bounds).  Those must be >= 0,
# and 0 is the prox of the zero function.  The library refuses a negative one with LMC_E_INVALID from the same table (eprox_params_ok in
# csrc/lmc_host.h; tests/test_gpu_eprox_accuracy.py holds the two against each other, parameter by parameter); the Python surface says which one first.
EPROX_PARAMS = {EPROX_LAPLACE: ("laplace", ("gamma",), (0,)), EPROX_UNCENTERED_LAPLACE: ("uncentered_laplace", ("gamma", "mu"), (0,)),
                EPROX_GAUSSIAN: ("gaussian", ("gamma",), (0,)), EPROX_GEN_GAUSSIAN_4_3: ("gen_gaussian_4_3", ("gamma",), (0,)),
                EPROX_GEN_GAUSSIAN_3_2: ("gen_gaussian_3_2", ("gamma",), (0,)), EPROX_GEN_GAUSSIAN_3: ("gen_gaussian_3", ("gamma",), (0,)),
                EPROX_GEN_GAUSSIAN_4: ("gen_gaussian_4", ("gamma",), (0,)), EPROX_HUBER: ("huber", ("gamma", "tau"), (0, 1)),
                EPROX_SMOOTHED_LAPLACE: ("smoothed_laplace", ("gamma",), (0,)), EPROX_EXP: ("exp", ("gamma",), (0,)),
                EPROX_GAMMA: ("gamma", ("omega", "kappa"), (0, 1)), EPROX_CHI: ("chi", ("kappa",), (0,)), EPROX_UNIFORM: ("uniform", ("omega",), (0,)),
                EPROX_TRIANGULAR: ("triangular", ("omega1", "omega2"), ()), EPROX_LAPLACE_CONJ: ("laplace_conj", ("gamma",), ())}


def check_eprox_params(kind, params):
    name, names, nonneg = EPROX_PARAMS[kind]
    for i in nonneg:
        if not float(params[i]) >= 0:
            raise ValueError(f"prox_{name}: {names[i]} is a weight and must be >= 0 (got {params[i]!r})")


class LMCError(RuntimeError):
    """A liblmc_atomi call returned a negative lmc_status."""

    def __init__(self, code, msg):
        super().__init__(f"liblmc_atomi error {code}: {msg}")
        self.code = code


class lmc_problem(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("H", C.c_int32), ("W", C.c_int32),
        ("data_kind", C.c_int32),
        ("sigma_f", C.c_float),
        # large PSF (data kinds 9 .. 11): size and origin of the kernel at h_host; the four bytes fill the alignment hole in front of y_dev
        ("psf_kh", C.c_uint8), ("psf_kw", C.c_uint8), ("psf_oy", C.c_uint8), ("psf_ox", C.c_uint8),
        ("y_dev", C.c_void_p),
        ("mask_dev", C.c_void_p),
        ("kh", C.c_int32), ("kw", C.c_int32), ("oy", C.c_int32), ("ox", C.c_int32),
        ("h_host", C.POINTER(C.c_float)),
        ("prior_kind", C.c_int32),
        ("prior_sigma", C.c_float),
        ("tv_niter", C.c_int32),
        ("tv_step", C.c_float),
        ("tv_betas_host", C.POINTER(C.c_float)),
        ("ncvx_kind", C.c_int32),
        ("ncvx_lambda", C.c_float),
        ("ncvx_gamma", C.c_float),
        ("ncvx_niter", C.c_int32),
        # ABI 2
        ("tv_lagged_output", C.c_int32),
        ("tv_rtol", C.c_float),
        ("step_variant", C.c_int32),
        ("implicit_tol", C.c_float),
        ("tv_warm", C.c_int32),
        # ABI 3
        ("ncvx_rtol", C.c_float),
        ("tv_exit_path", C.c_int32),
        ("iterations_per_launch", C.c_int32),
        ("moments_overlap", C.c_int32),
        ("moments_bg_workgroups", C.c_int32),
        ("graph_replay", C.c_int32),
        ("eprox_kind", C.c_int32), ("eprox_p0", C.c_float), ("eprox_p1", C.c_float), ("eprox_scale_mask", C.c_int32),
        ("psf_separable", C.c_int32),      # large PSF: 0 auto, 1 require, 2 forbid the two-pass form (fills the hole in front of prox_scale)
        ("prox_scale", C.c_void_p), ("prox_scale_chain_stride", C.c_int64), ("prox_scale_pixel_stride", C.c_int32),
        # box constraint (appended; ABI stays 4)
        ("box_enable", C.c_int32), ("box_lo", C.c_float), ("box_hi", C.c_float),
    ]


class lmc_myula_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("problem", lmc_problem),
        ("n_chains", C.c_int32),
        ("chain_offset", C.c_int64),
        ("tau", C.c_float), ("gamma", C.c_float), ("epsg", C.c_float),
        ("seed", C.c_uint64),
        ("noise_mode", C.c_int32),
        ("moments", C.c_int32),
        ("burn_in", C.c_int32),
        ("thin", C.c_int32),
    ]


class lmc_mch_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("problem", lmc_problem),
        ("n_channels", C.c_int32),
        ("mask_channel_stride", C.c_int64),
        ("n_chains", C.c_int32),
        ("chain_offset", C.c_int64),
        ("tau", C.c_float), ("gamma", C.c_float), ("epsg", C.c_float),
        ("seed", C.c_uint64),
        ("noise_mode", C.c_int32),
        ("moments", C.c_int32), ("burn_in", C.c_int32), ("thin", C.c_int32),
    ]


MAX_SGS_INNER = 16        # LMC_MAX_SGS_INNER


class lmc_sgs_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("problem", lmc_problem),
        ("n_chains", C.c_int32),
        ("chain_offset", C.c_int64),
        ("rho", C.c_float), ("tau", C.c_float), ("gamma", C.c_float), ("epsg", C.c_float),
        ("n_inner", C.c_int32),
        ("seed", C.c_uint64),
        ("noise_mode", C.c_int32),
        ("moments", C.c_int32), ("burn_in", C.c_int32), ("thin", C.c_int32),
    ]


class lmc_ulpda_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("problem", lmc_problem),
        ("n_chains", C.c_int32),
        ("chain_offset", C.c_int64),
        ("tau", C.c_float), ("mu", C.c_float), ("theta", C.c_float),
        ("gfirst", C.c_int32),
        ("cg_niter", C.c_int32),
        ("warm", C.c_int32),
        ("z_dev", C.c_void_p),
        ("seed", C.c_uint64),
        ("noise_mode", C.c_int32),
        ("moments", C.c_int32), ("burn_in", C.c_int32), ("thin", C.c_int32),
    ]


class lmc_sapg_config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("theta0", C.c_double), ("theta_min", C.c_double), ("theta_max", C.c_double),
        ("dim_eff", C.c_double),
        ("step_scale", C.c_double), ("step_exponent", C.c_double),
        ("warmup_iters", C.c_int32),
        ("n_updates", C.c_int32),
        ("iters_per_update", C.c_int32),
        ("average_from", C.c_int32),
    ]


_P = C.c_void_p
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_SIGNATURES = {
    "lmc_version": (C.c_int, []),
    "lmc_last_error": (C.c_char_p, []),
    "lmc_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lmc_hbm_copy_probe": (C.c_int, [C.c_size_t, C.c_int32, C.POINTER(C.c_float), _P]),
    "lmc_blur": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_psf_apply": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_psf_separable": (C.c_int, [_F, C.c_int32, C.c_int32, _F, _F]),
    "lmc_rfft2": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "lmc_irfft2": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "lmc_spectral_filter": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "lmc_spectral_tables": (C.c_int, [_D, _D, C.c_int32, C.c_int32, _F]),
    "lmc_sense_apply": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_sense_lipschitz": (C.c_double, [_F, C.c_int32, C.c_int32, C.c_int32]),
    "lmc_radon_apply": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _F, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_radon_tables": (C.c_int, [_F, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F]),
    "lmc_gradient": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "lmc_gradient_adjoint": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "lmc_fused_eval": (C.c_int, [C.POINTER(lmc_problem), _P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "lmc_l2_prox_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "lmc_l2_prox": (C.c_int, [C.POINTER(lmc_problem), _P, _P, C.c_int64, C.c_float, C.c_int32, C.c_int32, _P, _P]),
    "lmc_energies": (C.c_int, [C.POINTER(lmc_problem), _P, C.c_int64, _P, _P, _P]),
    "lmc_mymala_create": (C.c_int, [C.POINTER(lmc_myula_config), C.POINTER(_P)]),
    "lmc_sampler_get_acceptance": (C.c_int, [_P, _P, _P, _P]),
    "lmc_skrock_coefficients": (C.c_int, [C.c_int32, C.c_double, _D, _D, _D, _D]),
    "lmc_skrock_create": (C.c_int, [C.POINTER(lmc_myula_config), C.c_int32, C.c_float, C.POINTER(_P)]),
    "lmc_prior_statistic": (C.c_int, [C.POINTER(lmc_problem), _P, C.c_int64, _P, _P]),
    "lmc_sampler_set_prior_sigma": (C.c_int, [_P, C.c_float]),
    "lmc_sapg_dimension": (C.c_int, [C.POINTER(lmc_problem), _D, _D]),
    "lmc_sapg_update": (C.c_int, [C.POINTER(lmc_sapg_config), C.c_int64, C.c_double, C.c_double, _D]),
    "lmc_sampler_sapg": (C.c_int, [_P, C.POINTER(lmc_sapg_config), _P, _D, _D, _D, _P]),
    "lmc_set_cg_tolerance": (C.c_float, [C.c_float]),
    "lmc_chain_probes": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_haar_l1_prox": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, _P]),
    "lmc_wavelet_filter": (C.c_int, [C.c_int32, _D, C.POINTER(C.c_int32)]),
    "lmc_wavelet_apply": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "lmc_wavelet_l1_prox": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P]),
    "lmc_vtv_prox": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float, _F, C.c_int32, C.c_float, C.c_float, _P]),
    "lmc_vtv_value": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P]),
    "lmc_vtv_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 4),
    "lmc_tgv_prox": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float, _P]),
    "lmc_tgv_launch_iters": (C.c_int, []),
    "lmc_mch_create": (C.c_int, [C.POINTER(lmc_mch_config), C.POINTER(_P)]),
    "lmc_mch_destroy": (None, [_P]),
    "lmc_mch_set_state": (C.c_int, [_P, _P, _P]),
    "lmc_mch_get_state": (C.c_int, [_P, _P, _P]),
    "lmc_mch_step": (C.c_int, [_P, C.c_int32, _P, _P]),
    "lmc_mch_iteration": (C.c_int64, [_P]),
    "lmc_mch_set_iteration": (C.c_int, [_P, C.c_int64]),
    "lmc_mch_get_moments": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_mch_reset_moments": (C.c_int, [_P, _P]),
    "lmc_mch_energies": (C.c_int, [_P, _P, _P, _P]),
    "lmc_mch_noise": (C.c_int, [_P, C.c_int64, _P, _P]),
    "lmc_mch_kernel_name": (C.c_char_p, [_P]),
    "lmc_sgs_create": (C.c_int, [C.POINTER(lmc_sgs_config), C.POINTER(_P)]),
    "lmc_sgs_destroy": (None, [_P]),
    "lmc_sgs_set_state": (C.c_int, [_P, _P, _P]),
    "lmc_sgs_get_state": (C.c_int, [_P, _P, _P]),
    "lmc_sgs_step": (C.c_int, [_P, C.c_int32, _P, _P]),
    "lmc_sgs_iteration": (C.c_int64, [_P]),
    "lmc_sgs_set_iteration": (C.c_int, [_P, C.c_int64]),
    "lmc_sgs_get_moments": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_sgs_reset_moments": (C.c_int, [_P, _P]),
    "lmc_sgs_set_chain_groups": (C.c_int, [_P, C.c_int32]),
    "lmc_sgs_get_group_moments": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_sgs_energies": (C.c_int, [_P, _P, _P, _P, _P]),
    "lmc_sgs_noise": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P]),
    "lmc_sgs_kernel_name": (C.c_char_p, [_P]),
    "lmc_sgs_xstep": (C.c_int, [C.POINTER(lmc_problem), _P, _P, _P, C.c_int64, C.c_float, _P]),
    "lmc_dual_project": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P]),
    "lmc_prox_elementwise": (C.c_int, [C.c_int32, _P, _P, C.c_int64, _F, C.c_int32, _P]),
    "lmc_myula_create": (C.c_int, [C.POINTER(lmc_myula_config), C.POINTER(_P)]),
    "lmc_sampler_destroy": (None, [_P]),
    "lmc_sampler_set_state": (C.c_int, [_P, _P, _P]),
    "lmc_sampler_get_state": (C.c_int, [_P, _P, _P]),
    "lmc_sampler_step": (C.c_int, [_P, C.c_int32, _P, _P]),
    "lmc_sampler_iteration": (C.c_int64, [_P]),
    "lmc_sampler_set_iteration": (C.c_int, [_P, C.c_int64]),
    "lmc_sampler_get_moments": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_sampler_reset_moments": (C.c_int, [_P, _P]),
    "lmc_sampler_set_moment_scales": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    "lmc_sampler_get_block_moments": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_sampler_set_histogram": (C.c_int, [_P, C.c_int32, _P, _P]),
    "lmc_sampler_get_histogram": (C.c_int, [_P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_sampler_energies": (C.c_int, [_P, _P, _P, _P]),
    "lmc_sampler_noise": (C.c_int, [_P, C.c_int64, _P, _P]),
    "lmc_sampler_enable_timing": (C.c_int, [_P, C.c_int32]),
    "lmc_sampler_last_step_timing": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "lmc_sampler_kernel_name": (C.c_char_p, [_P]),
    "lmc_sampler_tv_exit_stats": (C.c_int, [_P, C.c_int32, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_set_step_variant": (C.c_int, [C.c_int32]),
    "lmc_ulpda_create": (C.c_int, [C.POINTER(lmc_ulpda_config), C.POINTER(_P)]),
    "lmc_sampler_set_dual": (C.c_int, [_P, _P, _P]),
    "lmc_sampler_get_dual": (C.c_int, [_P, _P, _P]),
    "lmc_sampler_set_steps": (C.c_int, [_P, C.c_float, C.c_float]),
    "lmc_rccl_available": (C.c_int, []),
    "lmc_rccl_unique_id": (C.c_int, [_P]),
    "lmc_rccl_comm_create": (C.c_int, [C.POINTER(_P), C.c_int32, C.c_int32, _P]),
    "lmc_rccl_comm_destroy": (C.c_int, [_P]),
    "lmc_allreduce_moments": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_allreduce_block_moments": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_allreduce_histogram": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_pixel_histogram": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "lmc_group_moments": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "lmc_sampler_set_chain_groups": (C.c_int, [_P, C.c_int32]),
    "lmc_sampler_get_group_moments": (C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_allreduce_group_moments": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_uint64), _P]),
    "lmc_cov_sketch_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "lmc_cov_sketch": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "lmc_sampler_set_cov_sketch": (C.c_int, [_P, C.c_int32, _P, _P]),
    "lmc_sampler_get_cov_sketch": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_uint64), _P]),
}
RCCL_UNIQUE_ID_BYTES = 128
VARIANTS = ["auto", "tile", "(removed)", "split", "point", "block", "rows", "pipe", "pipe2"]

_lib = None
_lock = threading.Lock()


def load(path: str | None = None):
    """Load liblmc_atomi.so (once).  torch is imported first so that the HIP runtime that
    PyTorch-ROCm ships (same soname, libamdhip64.so.7) is the one the library binds to --
    device pointers of torch tensors are then valid in our launches."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (HIP runtime first)
        p = path or os.environ.get("LMC_ATOMI_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise ImportError(
                f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C lmc_atomi_amd/csrc`).  lmc_atomi_amd has no CPU fallback.")
        lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
        v = lib.lmc_version()
        if v != ABI_VERSION:
            raise ImportError(f"liblmc_atomi ABI {v} != binding ABI {ABI_VERSION}")
        _lib = lib
        return lib


def check(rc: int):
    if rc != 0:
        raise LMCError(rc, load().lmc_last_error().decode("utf-8", "replace"))


def check_wavelet(dims, wavelet, levels):
    """``(p, levels)`` of a wavelet name on ``dims`` images; ``ValueError`` for what the library refuses with LMC_E_INVALID (include/lmc_atomi.h)."""
    if wavelet not in WAVELETS:
        raise ValueError(f"wavelet must be one of {sorted(WAVELETS)} (got {wavelet!r})")
    p, levels = WAVELETS[wavelet], int(levels)
    if not 1 <= levels <= MAX_WAVELET_LEVELS:
        raise ValueError(f"levels must be in 1 .. {MAX_WAVELET_LEVELS} (got {levels})")
    H, W = int(dims[0]), int(dims[1])
    if H % (1 << levels) or W % (1 << levels):
        raise ValueError(f"image sides must be multiples of 2^levels = {1 << levels} (got {H} x {W})")
    if (min(H, W) >> (levels - 1)) < 2 * p:
        raise ValueError(f"{levels} levels of {wavelet} need min(H, W) >> (levels - 1) >= {2 * p} (got {H} x {W}): the coarsest level must hold the filter")
    return p, levels


def check_fft_dims(dims):
    """``(H, W)`` as ints; ``ValueError`` unless both are powers of two in ``FFT_MIN .. FFT_MAX`` (the sides the LDS transforms are built for)."""
    try:
        H, W = int(dims[0]), int(dims[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError(f"dims must be a pair (H, W) (got {dims!r})") from None
    for n in (H, W):
        if not (FFT_MIN <= n <= FFT_MAX) or n & (n - 1):
            raise ValueError(f"the transforms take sides that are powers of two in {FFT_MIN} .. {FFT_MAX} (got {H} x {W})")
    return H, W


def vtv_plan(dims, n_channels, niter):
    """``(tile_h, tile_w, iters_per_launch, n_launches)`` of the vectorial-TV prox kernel (lmc_vtv_plan; host only, no device needed)."""
    out = [C.c_int32() for _ in range(4)]
    check(load().lmc_vtv_plan(int(dims[0]), int(dims[1]), int(n_channels), int(niter), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def tgv_launch_iters():
    """The iterations one launch of the TGV prox kernel holds (lmc_tgv_launch_iters; host only): a prox of more runs as chained launches."""
    return int(load().lmc_tgv_launch_iters())


def exported_symbols():
    return sorted(_SIGNATURES)
