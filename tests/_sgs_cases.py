"""The configurations of lmc_sgs_create that tests/test_sgs_api.py (host only) and tests/test_gpu_sgs.py (with device pointers) hold against its refusals:
a configuration the library accepts, the fields that make it LMC_E_UNSUPPORTED with a word of the message, and the fields that make it LMC_E_INVALID."""
import ctypes as C

LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
FAKE = 4096      # a non-NULL address that no refused call reads


def sgs_config(**fields):
    """A configuration the library accepts up to the first device call; `fields`: lmc_problem fields (by name) and config fields (prefixed cfg_)."""
    from lmc_atomi_amd import _capi
    cfg = _capi.lmc_sgs_config()
    cfg.struct_size = C.sizeof(_capi.lmc_sgs_config)
    p = cfg.problem
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W, p.data_kind, p.sigma_f, p.y_dev = 16, 16, _capi.DATA_IDENTITY, 1.0, FAKE
    p.prior_kind, p.prior_sigma = _capi.PRIOR_L1, 0.5
    cfg.n_chains, cfg.rho, cfg.tau, cfg.gamma, cfg.epsg, cfg.n_inner, cfg.thin = 2, 1.0, 0.1, 0.5, 1.0, 1, 1
    for k, v in fields.items():
        if k.startswith("cfg_"):
            setattr(cfg, k[4:], v)
        else:
            setattr(p, k, v)
    return cfg


def create(cfg):
    from lmc_atomi_amd import _dev
    h = C.c_void_p()
    rc = _dev.lib().lmc_sgs_create(C.byref(cfg), C.byref(h))
    assert not h.value
    return rc, _dev.lib().lmc_last_error().decode()


TAPS = (C.c_float * 9)(*([1.0 / 9] * 9))
ANGLES = (C.c_float * 4)(0.0, 0.5, 1.0, 1.5)
UNSUPPORTED = [
    (dict(data_kind=2, kh=3, kw=3, oy=1, ox=1, h_host=TAPS), "PeriodicConvolve2D"),                    # zero-padded blur
    (dict(data_kind=8, kh=3, kw=3, oy=1, ox=1, h_host=TAPS), "PeriodicConvolve2D"),                    # weighted, on a blur
    (dict(data_kind=9, psf_kh=3, psf_kw=3, psf_oy=1, psf_ox=1, h_host=TAPS), "PeriodicConvolve2D"),    # large PSF
    (dict(data_kind=16, kh=4, kw=16, h_host=ANGLES), "Radon"),
    (dict(data_kind=4), "not Gaussian"),                                                                # Poisson
    (dict(data_kind=6, mask_dev=FAKE), "not Gaussian"),
    (dict(data_kind=13), "not Gaussian"),                                                               # Huber
    (dict(ncvx_kind=1, ncvx_gamma=1.0), "ncvx_kind"),
    (dict(prior_kind=3, tv_niter=10, tv_rtol=1e-4), "tv_rtol"),
    (dict(prior_kind=3, tv_niter=3, tv_warm=1), "tv_warm"),
    (dict(prox_scale=FAKE), "prox_scale"),
    (dict(prior_kind=8, tv_niter=10), "LMC_PRIOR_VTV"),
]
INVALID = [dict(cfg_rho=0.0), dict(cfg_rho=-1.0), dict(cfg_rho=float("nan")), dict(cfg_rho=float("inf")), dict(cfg_tau=0.0), dict(cfg_tau=float("inf")),
           dict(cfg_gamma=-0.5), dict(cfg_gamma=float("nan")), dict(cfg_n_inner=0), dict(cfg_n_inner=17), dict(cfg_n_chains=0), dict(cfg_struct_size=8),
           dict(data_kind=12, H=12, W=16), dict(data_kind=12, H=16, W=4), dict(data_kind=12, H=2048, W=16)]
