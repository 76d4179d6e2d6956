"""Sampler entry points -- drop-ins for the reference's ``algs.py``.

``MoreauYosidaUnadjustedLangevin`` keeps the reference signature (algs.py:477-478) and return
value (``ndarray (niter, n)`` of all iterates) for one chain, and adds keyword-only extensions
for what the reference lacks: many chains per GPU, sharding-invariant counter-based noise,
posterior moments with burn-in / thinning, per-chain energy diagnostics.

The per-iteration update runs entirely in hand-written HIP kernels behind the C ABI
(include/lmc_atomi.h); torch tensors are HBM containers only.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch
from numpy.random import default_rng

from . import _capi, _dev
from .proximal import L2, VectorialTV, _Problem
from .operators import Convolve2D, Diagonal, Identity
from .summaries import (ACCUMULATOR_KEYWORDS, HIST_MAX_BINS, MAX_CHAIN_GROUPS, MAX_COV_PROBES, MOMENT_SCALES, CovSketch, GroupMCSE,  # noqa: F401
                        _check_accumulators, _check_chain_groups, _check_cov_sketch, _check_histogram, _check_moment_scales, _cov_summary,
                        _group_summaries, _hist_arrays, _hist_host, _hist_summaries, _host_array, _scale_summaries, block_mean_var,
                        cov_from_sketch, cov_sketch, group_moments, hist_exceedance, hist_quantiles, mcse_from_group_moments,
                        mean_var_from_moments, pixel_histogram, random_probes)


def _prior_descriptor(proxg):
    if proxg is None:
        return {"prior_kind": _capi.PRIOR_NONE}
    fn = getattr(proxg, "prior_descriptor", None)
    if fn is None:
        raise NotImplementedError(
            f"{type(proxg).__name__} has no device functor (prior_descriptor()); new proxes are added as "
            "functors compiled into liblmc_atomi -- there is no CPU fallback")
    return fn()


def _refuse_box(prior, who, why):
    """``NotImplementedError`` for a prior with ``bounds=`` where ``who`` has no box-constrained form (before any handle exists)."""
    if prior.get("box") is not None:
        raise NotImplementedError(f"{who} does not take a prior with bounds: {why}")


def _refuse_eprox(prior, who, why):
    """``NotImplementedError`` for a closed-form prior (``LMC_PRIOR_EPROX``: a prox and no value) where ``who`` needs g(x) (before any handle exists)."""
    if prior.get("prior_kind") == _capi.PRIOR_EPROX:
        raise NotImplementedError(f"{who} does not take a closed-form prior (ElementwiseProx, Laplace, Huber, ...): {why}")


# The data terms with step kernels of their own: (kinds, name in messages, what the user wrote -- appended where a sampler refuses the term outright --, the
# kind on a large PSF whose remaining refusals are _refuse_psf's, or None).  The kinds are disjoint: at most one row speaks.
_TERMS = {
    "poisson": (_capi.POISSON_KINDS, "the Poisson data term", "", None),
    "wl2": (_capi.WL2_KINDS, "the weighted Gaussian data term", " (L2 with weights)", None),
    "huber": (_capi.HUBER_KINDS, "the Huber data term", " (HuberLoss)", _capi.DATA_HUBER_PSF),
}


def _refuse_term(data, prior, opts, who=None):
    """``NotImplementedError`` for what the library refuses with a Poisson, weighted Gaussian (``L2(weights=...)``) or Huber (``HuberLoss``) data term
    (``LMC_E_UNSUPPORTED`` in include/lmc_atomi.h), before a handle exists.  ``who``: term -> (name, why) of a sampler that has no form of that term at all."""
    kind = data.get("data_kind")
    for term, (kinds, name, label, psf_kind) in _TERMS.items():
        if kind not in kinds:
            continue
        if who and term in who:
            raise NotImplementedError(f"{who[term][0]} does not take {name}{label}: {who[term][1]}")
        if kind == psf_kind:
            return
        if prior.get("prior_kind") == _capi.PRIOR_HAAR_L1:
            raise NotImplementedError(f"{name} with the Haar-l1 prior (WaveletL1) is not built")
        if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
            raise NotImplementedError(f"{name} runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
        if prior.get("tv_warm") or opts.get("tv_warm"):
            raise NotImplementedError(f"{name} has no warm-started TV dual: warm / tv_warm must be off")
        v = opts.get("step_variant", 0) or 0
        v = _capi.VARIANTS.index(v) if isinstance(v, str) else int(v)
        if v not in (0, 1, 7):
            raise NotImplementedError(f"step-kernel variant {_capi.VARIANTS[v]!r} has no form of {name}: 'auto', 'tile' or 'pipe' (where it covers the problem)")


def _refuse_psf(data, prior, opts, who=None):
    """The same for a large PSF (``Op = PSF(...)``, ``LMC_DATA_PSF`` / ``POISSON_PSF`` / ``WL2_PSF`` / ``HUBER_PSF``)."""
    if data.get("data_kind") not in _capi.PSF_KINDS:
        return
    if who is not None:
        raise NotImplementedError(f"{who[0]} does not take a large PSF (Op = PSF(...)): {who[1]}")
    if data.get("ncvx_kind", _capi.NCVX_NONE) != _capi.NCVX_NONE:
        raise NotImplementedError("a large PSF has no non-convex form")
    if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
        raise NotImplementedError("a large PSF runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
    if prior.get("tv_warm") or opts.get("tv_warm"):
        raise NotImplementedError("a large PSF has no warm-started TV dual: warm / tv_warm must be off")


def _refuse_spectral(data, prior, opts, who=None):
    """The same for the Fourier-domain data term (``Op = FourierSampling(...)`` / ``PeriodicConvolve2D(...)``, ``LMC_DATA_SPECTRAL``)."""
    if data.get("data_kind") != _capi.DATA_SPECTRAL:
        return
    if who is not None:
        raise NotImplementedError(f"{who[0]} does not take the Fourier-domain data term (Op = FourierSampling / PeriodicConvolve2D): {who[1]}")
    if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
        raise NotImplementedError("the Fourier-domain data term runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
    if prior.get("tv_warm") or opts.get("tv_warm"):
        raise NotImplementedError("the Fourier-domain data term has no warm-started TV dual: warm / tv_warm must be off")


def _refuse_radon(data, prior, opts, who=None):
    """The same for the Radon operator (``Op = Radon(...)``, ``LMC_DATA_RADON`` / ``POISSON_RADON`` / ``WL2_RADON`` / ``HUBER_RADON``)."""
    if data.get("data_kind") not in _capi.RADON_KINDS:
        return
    if who is not None:
        raise NotImplementedError(f"{who[0]} does not take the Radon operator (Op = Radon(...)): {who[1]}")
    if data.get("ncvx_kind", _capi.NCVX_NONE) != _capi.NCVX_NONE:
        raise NotImplementedError("the Radon operator has no non-convex form")
    if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
        raise NotImplementedError("the Radon operator runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
    if prior.get("tv_warm") or opts.get("tv_warm"):
        raise NotImplementedError("the Radon operator has no warm-started TV dual: warm / tv_warm must be off")


def _refuse_sense(data, prior, opts, who=None):
    """The same for the multi-coil SENSE data term (``Op = MultiCoilFourierSampling(...)``, ``LMC_DATA_SENSE``)."""
    if data.get("data_kind") != _capi.DATA_SENSE:
        return
    if who is not None:
        raise NotImplementedError(f"{who[0]} does not take the multi-coil SENSE data term (Op = MultiCoilFourierSampling): {who[1]}")
    if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
        raise NotImplementedError("the multi-coil SENSE data term runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
    if prior.get("tv_warm") or opts.get("tv_warm"):
        raise NotImplementedError("the multi-coil SENSE data term has no warm-started TV dual: warm / tv_warm must be off")


def _refuse_vtv(proxg, who):
    """``NotImplementedError`` for the vectorial TV prior where ``who`` samples single-plane images (before any handle exists)."""
    if isinstance(proxg, VectorialTV):
        raise NotImplementedError(f"{who} does not take VectorialTV: the multi-channel prior is built for MultichannelMYULASampler (and "
                                  "MoreauYosidaUnadjustedLangevin, which routes to it) only -- MYMALA, SK-ROCK, ULPDA and the estimation of the prior "
                                  "weight are not built for it")


def _refuse_tgv(prior, who, why):
    """``NotImplementedError`` for the TGV prior (``LMC_PRIOR_TGV``: a prox and no value) where ``who`` needs g(x) or a scalar-free prox (before any handle exists)."""
    if prior.get("prior_kind") == _capi.PRIOR_TGV:
        raise NotImplementedError(f"{who} does not take the TGV prior: {why}")


def _data_descriptor(proxf):
    if proxf is None:
        return {"data_kind": _capi.DATA_NONE}
    fn = getattr(proxf, "descriptor", None)
    if fn is None:
        raise NotImplementedError(f"{type(proxf).__name__} has no device functor (descriptor())")
    return fn()


def _dims_of(dims, *objs):
    """``dims`` as given, else the ``dims`` of the first of ``objs`` that has them; ``ValueError`` when none does."""
    if dims is None:
        for o in objs:
            dims = dims or getattr(o, "dims", None)
    if dims is None:
        raise ValueError("image shape unknown: pass dims=(ny, nx)")
    return dims


def _accumulator_keywords(ns, many, n_chains, dims):
    """The accumulator keywords of a driver (``ns``: its ``locals()``) as the one mapping it hands to its sampler, after the driver's own checks:
    they belong to the many-chain form, the chain groups need a chain each, the probes must fit the image."""
    kw = {k: ns[k] for k in ACCUMULATOR_KEYWORDS}
    if kw["moment_scales"] and not many:
        raise ValueError("moment_scales belongs to the many-chain form (n_chains=C): the reference form keeps every iterate instead")
    if (kw["hist_bins"] is not None or kw["hist_range"] is not None) and not many:
        raise ValueError("hist_bins / hist_range belong to the many-chain form (n_chains=C): the reference form keeps every iterate instead")
    if kw["chain_groups"] is not None and not many:
        raise ValueError("chain_groups belongs to the many-chain form (n_chains=C): one chain has no groups to compare")
    _check_chain_groups(kw["chain_groups"], True, n_chains)
    if (kw["cov_probes"] is not None or kw["cov_center"] is not None) and not many:
        raise ValueError("cov_probes / cov_center belong to the many-chain form (n_chains=C): the reference form keeps every iterate instead")
    _check_cov_sketch(kw["cov_probes"], kw["cov_center"], True, dims)
    return kw


def _comm(rccl_comm):
    """An ``ncclComm_t`` given as an integer, a ``c_void_p`` or ``None`` (a job of one rank), as the ``c_void_p`` the C ABI takes."""
    return rccl_comm if isinstance(rccl_comm, C.c_void_p) else C.c_void_p(int(rccl_comm or 0))


class SAPGResult:
    """Outcome of a SAPG estimation: ``theta`` (the averaged weight), ``theta_trace`` (``n_updates + 1`` float64, entry 0 = theta0),
    ``stat_trace`` (``n_updates`` float64: the mean over the chains of the prior value with weight 1 at every update), ``dim_eff`` and
    ``degree`` as used; ``state`` only from :func:`EstimatePriorWeight`."""

    def __init__(self, theta, theta_trace, stat_trace, dim_eff, degree, state=None):
        self.theta = theta
        self.theta_trace = theta_trace
        self.stat_trace = stat_trace
        self.dim_eff = dim_eff
        self.degree = degree
        self.state = state


def _check_sapg(rc):
    """Status of a weight / SAPG call: LMC_E_INVALID -> ValueError, LMC_E_UNSUPPORTED -> NotImplementedError (the module's convention)."""
    if rc in (-1, -2):
        msg = _dev.lib().lmc_last_error().decode("utf-8", "replace")
        raise (ValueError if rc == -1 else NotImplementedError)(msg)
    _capi.check(rc)


def _prior_weight(proxg):
    w = _prior_descriptor(proxg).get("prior_sigma")
    if w is None:
        raise NotImplementedError(f"{type(proxg).__name__} has no weight to estimate")
    return float(w)


def _stat_problem(proxg, dims):
    """The part of an ``lmc_problem`` the prior statistic and its dimension read: no device buffer."""
    p = _capi.lmc_problem()
    p.struct_size = C.sizeof(_capi.lmc_problem)
    p.H, p.W = int(dims[0]), int(dims[1])
    d = _prior_descriptor(proxg)
    p.prior_kind = d["prior_kind"]
    if p.prior_kind == _capi.PRIOR_WAVELET_L1:      # the kind's two parameters: levels and p
        p.tv_niter, p.eprox_kind = int(d["wavelet_levels"]), int(d["wavelet_p"])
    return p


def sapg_dimension(proxg, dims=None):
    """``(dim_eff, degree)`` the SAPG update uses by default for the prior ``proxg`` on ``dims`` images: l1 ``(H W, 1)``, l2 ``(H W, 2)``,
    TV ``(H W - 1, 1)``, Haar-l1 ``(H W - (H/8)(W/8), 1)``, wavelet-l1 over L levels ``(H W - (H >> L)(W >> L), 1)``.  Needs no GPU; a prior without a value raises ``NotImplementedError``."""
    if dims is None:
        dims = getattr(proxg, "dims", None)
    if dims is None:
        raise ValueError("image shape unknown: pass dims=(ny, nx)")
    d, k = C.c_double(), C.c_double()
    _check_sapg(_dev.lib().lmc_sapg_dimension(C.byref(_stat_problem(proxg, dims)), C.byref(d), C.byref(k)))
    return d.value, k.value


def _sapg_config(n_updates, theta_bounds, theta0, warmup=0, iters_per_update=1, step_scale=10., step_exponent=0.8, average_from=None, dim_eff=None):
    """A checked ``lmc_sapg_config``; every argument error is a ``ValueError`` raised here, before any device call."""
    try:
        lo, hi = (float(v) for v in theta_bounds)
    except (TypeError, ValueError):
        raise ValueError("theta_bounds must be a pair (lo, hi)") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"theta_bounds must satisfy 0 < lo <= hi (got {theta_bounds!r})")
    theta0 = float(theta0)
    if not lo <= theta0 <= hi:
        raise ValueError(f"theta0 = {theta0} lies outside theta_bounds = ({lo}, {hi})")
    if not 0.5 < float(step_exponent) <= 1.0:
        raise ValueError(f"step_exponent must be in (0.5, 1] (got {step_exponent})")
    if not (np.isfinite(step_scale) and float(step_scale) > 0.0):
        raise ValueError(f"step_scale must be > 0 (got {step_scale})")
    n_updates, warmup, iters_per_update = int(n_updates), int(warmup), int(iters_per_update)
    if n_updates < 1 or warmup < 0 or iters_per_update < 1:
        raise ValueError("n_updates >= 1, warmup >= 0 and iters_per_update >= 1 are required")
    average_from = n_updates // 2 if average_from is None else int(average_from)
    if not 0 <= average_from < n_updates:
        raise ValueError(f"average_from must be in 0 .. n_updates - 1 (got {average_from})")
    dim_eff = 0.0 if dim_eff is None else float(dim_eff)
    if not (np.isfinite(dim_eff) and dim_eff >= 0.0):
        raise ValueError(f"dim_eff must be > 0, or None for the default (got {dim_eff})")
    cfg = _capi.lmc_sapg_config()
    cfg.struct_size = C.sizeof(_capi.lmc_sapg_config)
    cfg.theta0, cfg.theta_min, cfg.theta_max = theta0, lo, hi
    cfg.dim_eff = dim_eff
    cfg.step_scale, cfg.step_exponent = float(step_scale), float(step_exponent)
    cfg.warmup_iters, cfg.n_updates, cfg.iters_per_update, cfg.average_from = warmup, n_updates, iters_per_update, average_from
    return cfg


def sapg_update(theta, gbar, n, dim_eff, degree=1.0, theta_bounds=(1e-3, 1e2), step_scale=10., step_exponent=0.8):
    """One SAPG update on the host (``lmc_sapg_update``, the function the device kernel is compiled from): ``theta_{n+1}`` from ``theta_n``, the
    mean prior value ``gbar`` and the 0-based update index ``n``.  Needs no GPU.  The library's entry point is the degree-1 update; a prior of
    degree k is the same step with ``step_scale / k`` and ``k gbar``."""
    k = float(degree)
    if not k > 0.0:
        raise ValueError("degree must be > 0")
    if not float(dim_eff) > 0.0:
        raise ValueError("dim_eff must be > 0")
    cfg = _sapg_config(1, theta_bounds, theta_bounds[0], step_scale=float(step_scale) / k, step_exponent=step_exponent, dim_eff=dim_eff)
    out = C.c_double()
    _check_sapg(_dev.lib().lmc_sapg_update(C.byref(cfg), int(n), float(theta), k * float(gbar), C.byref(out)))
    return out.value


def prior_statistic(proxg, x, dims=None):
    """``g(x_i)`` with weight 1 for every image of ``x`` (float64 tensor in HBM, one entry per image): what the SAPG update averages over the
    chains.  One streaming read, no data term; every image is summed in a fixed order."""
    if dims is None:
        dims = getattr(proxg, "dims", None)
    if dims is None:
        if not (hasattr(x, "shape") and len(x.shape) >= 2):
            raise ValueError("image shape unknown: pass dims=(ny, nx)")
        dims = tuple(x.shape[-2:])
    p = _stat_problem(proxg, dims)
    xt = _dev.to_dev(x)
    n = p.H * p.W
    if xt.numel() % n or xt.numel() == 0:
        raise ValueError(f"operand of shape {tuple(xt.shape)} is not a batch of {tuple(dims)} images")
    out = torch.empty(xt.numel() // n, dtype=torch.float64, device=xt.device)
    with torch.cuda.device(xt.device):
        _check_sapg(_dev.lib().lmc_prior_statistic(C.byref(p), _dev.ptr(xt), xt.numel() // n, _dev.ptr(out), _dev.stream_ptr()))
    return out


class MYULASampler:
    """Many-chain MYULA on one GPU: owns an ``lmc_sampler`` handle.

    State layout in HBM: ``[n_chains, H, W]`` fp32.  ``chain_offset`` is the global id of local
    chain 0; the noise of a chain depends only on (seed, iteration, global chain id, pixel), so
    any sharding of the chains over GPUs reproduces the same trajectories.
    """

    def __init__(self, proxf, proxg, dims, n_chains=1, tau=None, gamma=0.1, epsg=1.0, seed=0,
                 chain_offset=0, noise="philox", moments=False, burn_in=0, thin=1, device=None, variant=None, tv_warm=None, policy=None,
                 moment_scales=None, hist_bins=None, hist_range=None, chain_groups=None, cov_probes=None, cov_center=None):
        """``variant``: step-kernel variant of THIS sampler ('auto' | 'tile' | 'split' | 'point' | 'block' | 'rows' | 'pipe' | 'pipe2'; None = the
        library default, :func:`set_step_variant`).  ``tv_warm``: carry the TV dual between iterations (see :class:`TV`; None = as
        ``proxg.warm`` says).  ``moment_scales``: block sizes out of (2, 4, 8, 16) whose block sums get second moments of their own over the kept samples
        (:meth:`block_moments`; needs ``moments=True``).  ``hist_bins`` (1 .. 62) with ``hist_range=(lo, hi)``, each a scalar or an ``[H, W]`` array:
        a histogram per pixel over the kept samples (:meth:`histogram`, :func:`hist_quantiles`; needs ``moments=True``) -- a short pilot run gives
        ``mean`` and ``var``, and ``(mean - 5 sqrt(var), mean + 5 sqrt(var))`` is then a range whose 62 bins resolve 0.16 standard deviations.
        ``chain_groups=G`` (2 .. 64): the sums of x and x^2 per pixel and chain group over the kept samples, the group of a chain being its global id
        mod G (:meth:`group_moments`, :func:`mcse_from_group_moments`: Monte-Carlo error and ESS maps; needs ``moments=True``).
        ``cov_probes`` (``[k, H, W]`` or ``[k, H*W]``, k <= 32) with ``cov_center`` (``[H, W]`` or flat, None = 0; best the mean of a pilot run): the
        covariance sketch over the kept samples -- ``Y = sum t d``, ``s = sum t``, ``Q = sum t t^T`` with ``d = x - cov_center`` and ``t = cov_probes . d``
        (:meth:`cov_sketch`, :func:`cov_from_sketch`: the covariance of every pixel with every projection, of region fluxes, Nystrom uncertainty modes;
        needs ``moments=True``).
        Every call on the sampler runs on ``device`` whatever the current device is."""
        acc = _check_accumulators(locals(), moments, dims)      # before anything touches the proxes
        _refuse_vtv(proxg, type(self).__name__)
        if tau is None:
            raise NotImplementedError("tau=None (backtracking) is not implemented by the reference loop either")
        if self._box_refusal is not None:
            _refuse_box(_prior_descriptor(proxg), *self._box_refusal)
        if self._eprox_refusal is not None:
            _refuse_eprox(_prior_descriptor(proxg), *self._eprox_refusal)
            _refuse_tgv(_prior_descriptor(proxg), self._eprox_refusal[0], "its value g(x) is a minimisation over the auxiliary field and is not built, so the "
                        "Metropolis target exp(-f - epsg g) cannot be evaluated; use MYULA or SK-ROCK")
        if np.asarray(epsg).size > 1 and _prior_descriptor(proxg).get("prior_kind") == _capi.PRIOR_WAVELET_L1:
            raise NotImplementedError("array-valued epsg is built for the closed-form priors only: the wavelet-l1 prior takes a scalar epsg")
        if np.asarray(epsg).size > 1:
            _refuse_tgv(_prior_descriptor(proxg), "array-valued epsg", "it is built for the closed-form priors only; TGV takes a scalar epsg")
        if tv_warm and _prior_descriptor(proxg).get("box") is not None:
            raise NotImplementedError("a prior with bounds has no warm-started dual: tv_warm must be off")
        self.dims = (int(dims[0]), int(dims[1]))
        self.n_chains = int(n_chains)
        self.device = _dev.device(device)
        self.proxf, self.proxg = proxf, proxg
        opts = {"step_variant": variant or 0}
        if tv_warm is not None:
            opts["tv_warm"] = bool(tv_warm)
        # launch policy of this sampler (lmc_problem, ABI 3): dict with any of iterations_per_launch (0 auto / 1 / 2), moments_overlap (0 auto /
        # 1 / -1), moments_bg_workgroups, tv_exit_path (1 = the pass-by-pass early exit); graph_replay is accepted and has no effect
        opts.update(policy or {})
        self.epsg = epsg
        if np.asarray(epsg).size > 1:      # array-valued epsg (algs.py:509,539-542): the prox parameter epsg * gamma is an array that the prox broadcasts
            opts["prox_scale"] = self._epsg_array(epsg)
            epsg = 1.0
        _refuse_term(_data_descriptor(proxf), _prior_descriptor(proxg), opts, self._term_refusal)
        _refuse_psf(_data_descriptor(proxf), _prior_descriptor(proxg), opts, self._psf_refusal)
        _refuse_spectral(_data_descriptor(proxf), _prior_descriptor(proxg), opts, self._spectral_refusal)
        _refuse_radon(_data_descriptor(proxf), _prior_descriptor(proxg), opts, self._radon_refusal)
        _refuse_sense(_data_descriptor(proxf), _prior_descriptor(proxg), opts, self._sense_refusal)
        self._problem = _Problem(self.dims, _data_descriptor(proxf), _prior_descriptor(proxg), self.device, options=opts)
        self.prior_weight = float(self._problem.c.prior_sigma)      # follows set_prior_weight / estimate_prior_weight
        cfg = _capi.lmc_myula_config()
        cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
        cfg.problem = self._problem.c
        cfg.n_chains = self.n_chains
        cfg.chain_offset = int(chain_offset)
        cfg.tau, cfg.gamma, cfg.epsg = float(tau), float(gamma), float(epsg)
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.noise_mode = {"philox": _capi.NOISE_PHILOX, "injected": _capi.NOISE_INJECTED, "none": _capi.NOISE_NONE}[noise]
        cfg.moments = 1 if moments else 0
        cfg.burn_in = int(burn_in)
        cfg.thin = int(thin)
        self.noise_mode = noise
        self.moments_on = bool(moments)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._create(cfg)
        if rc == -2 and self._problem.c.data_kind in _capi.POISSON_KINDS + _capi.WL2_KINDS + _capi.HUBER_KINDS + _capi.PSF_KINDS + (_capi.DATA_SPECTRAL,) + _capi.RADON_KINDS:      # (no handle exists: e.g. variant='pipe' on a problem the pipeline does not cover)
            raise NotImplementedError(_dev.lib().lmc_last_error().decode())
        _capi.check(rc)
        self._attach_accumulators(acc)

    _create_fn = "lmc_myula_create"
    _box_refusal = None          # (who, why) of a subclass that has no box-constrained form: raised before a handle exists
    _term_refusal = None         # the same for the data terms of _TERMS: term -> (who, why)
    _psf_refusal = None          # the same for a large PSF
    _spectral_refusal = None     # the same for the Fourier-domain data term
    _radon_refusal = None        # the same for the Radon operator
    _sense_refusal = None        # the same for the multi-coil SENSE data term
    _eprox_refusal = None        # the same for a closed-form prior (a prox without a value)

    def _create(self, cfg):
        return getattr(_dev.lib(), self._create_fn)(C.byref(cfg), C.byref(self._h))

    moment_scales = ()
    hist_bins = hist_lo = hist_scale = None
    chain_groups = None
    cov_k = cov_probes = cov_center = None
    prior_weight = None

    def _attach_accumulators(self, acc):
        """``acc``: (scales, hist, groups, cov) as :func:`_check_accumulators` returns them, onto the created handle.  The library copies lo / scale
        and probes / centre; the sampler keeps fp32 device copies of them for :func:`hist_quantiles` and :func:`cov_from_sketch`."""
        scales, hist, groups, cov = acc
        lib = _dev.lib()
        with torch.cuda.device(self.device):
            if scales:
                _capi.check(lib.lmc_sampler_set_moment_scales(self._h, len(scales), (C.c_int32 * len(scales))(*scales)))
            self.moment_scales = tuple(scales)
            if hist is not None:
                B, lo_d, sc_d = hist[0], _dev.to_dev(hist[1], self.device), _dev.to_dev(hist[2], self.device)
                torch.cuda.current_stream().synchronize()
                _capi.check(lib.lmc_sampler_set_histogram(self._h, B, _dev.ptr(lo_d), _dev.ptr(sc_d)))
                self.hist_bins, self.hist_lo, self.hist_scale = B, lo_d, sc_d
            if groups is not None:
                _capi.check(lib.lmc_sampler_set_chain_groups(self._h, int(groups)))
                self.chain_groups = int(groups)
            if cov is not None:
                k, P, m = cov
                P_d = _dev.to_dev(P, self.device).reshape((k,) + self.dims)
                m_d = None if m is None else _dev.to_dev(m, self.device).reshape(self.dims)
                torch.cuda.current_stream().synchronize()
                _capi.check(lib.lmc_sampler_set_cov_sketch(self._h, k, _dev.ptr(P_d), _dev.ptr(m_d)))
                self.cov_k, self.cov_probes, self.cov_center = k, P_d, m_d

    def _epsg_array(self, epsg):
        """Device copy + (chain, pixel) strides of an array-valued ``epsg``.  The reference hands ``epsg * gamma`` to ``proxg.prox`` (algs.py:569), whose
        closed forms broadcast it against ``x``: one weight per pixel of a flattened image (``x`` of shape ``(n,)``), one per right-hand side = per chain
        (``x`` of shape ``(n, nrhs)``, ``epsg`` of shape ``(nrhs,)``), or both.  Here: ``(H*W,)`` / ``(H, W)`` per pixel, ``(n_chains,)`` per chain,
        ``(n_chains, H*W)`` / ``(n_chains, H, W)`` both."""
        e = np.asarray(epsg, dtype=np.float32)
        n = self.dims[0] * self.dims[1]
        if e.size == n and e.shape in ((n,), self.dims):
            cs, ps = 0, 1
        elif e.shape == (self.n_chains,):
            cs, ps = 1, 0
        elif e.size == self.n_chains * n and e.shape[0] == self.n_chains:
            cs, ps = n, 1
        else:
            raise ValueError(f"epsg of shape {e.shape} matches neither the image {self.dims}, nor the {self.n_chains} chains, nor both")
        return _dev.to_dev(np.ascontiguousarray(e.ravel()), self.device), cs, ps

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _dev.lib().lmc_sampler_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ---------------------------------------------------------------------------
    @property
    def shape(self):
        return (self.n_chains,) + self.dims

    def set_state(self, x):
        xt = _dev.to_dev(x, self.device)
        n = self.dims[0] * self.dims[1]
        if xt.numel() == n:                       # one image: broadcast to every chain (x0 of algs.py:559)
            xt = xt.reshape(1, *self.dims).expand(self.shape).contiguous()
        if xt.numel() != self.n_chains * n:
            raise ValueError(f"state of shape {tuple(xt.shape)} does not match {self.shape}")
        _capi.check(_dev.lib().lmc_sampler_set_state(self._h, _dev.ptr(xt), _dev.stream_ptr(self.device)))
        torch.cuda.current_stream(self.device).synchronize()  # xt may be a temporary

    def get_state(self, out=None):
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_sampler_get_state(self._h, _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    @property
    def iteration(self):
        return int(_dev.lib().lmc_sampler_iteration(self._h))

    @iteration.setter
    def iteration(self, it):
        _capi.check(_dev.lib().lmc_sampler_set_iteration(self._h, int(it)))

    # -- hot loop ------------------------------------------------------------------------
    def step(self, n_iters=1, noise=None):
        """Run ``n_iters`` iterations of algs.py:564-570 on every chain.  ``noise`` (only with
        noise='injected'): ``[n_iters, n_chains, H, W]``."""
        nt = None
        if noise is not None:
            nt = _dev.to_dev(noise, self.device)
            if nt.numel() != n_iters * self.n_chains * self.dims[0] * self.dims[1]:
                raise ValueError("noise must have shape [n_iters, n_chains, H, W]")
        _capi.check(_dev.lib().lmc_sampler_step(self._h, int(n_iters), _dev.ptr(nt), _dev.stream_ptr(self.device)))
        if nt is not None:
            torch.cuda.current_stream(self.device).synchronize()

    def enable_timing(self, on=True):
        """Bracket every step-kernel launch with a HIP event pair on the launch stream."""
        _capi.check(_dev.lib().lmc_sampler_enable_timing(self._h, 1 if on else 0))

    def last_step_timing(self):
        """(summed step-kernel milliseconds, launches) of the last :meth:`step` call."""
        ms, n = C.c_float(), C.c_int32()
        _capi.check(_dev.lib().lmc_sampler_last_step_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @property
    def kernel_name(self):
        return _dev.lib().lmc_sampler_kernel_name(self._h).decode()

    def tv_exit_stats(self, which="prior"):
        """Early-exit statistics of the device path (``TV(rtol > 0)`` / ``L2_ncvx_tv(rtol > 0)``): ``(passes, reruns)`` -- the loop pass each
        chain's latest prox left in (int32 tensor, ``niter`` = it ran out of passes) and the number of chain runs that had to be repeated
        after rounds 1 / 2 / 3 / 4 since the sampler was created (``which``: 'prior' = the TV prior's prox, 'ncvx' = the ME-TV inner prox)."""
        passes = torch.empty(self.n_chains, dtype=torch.int32, device=self.device)
        rr = (C.c_uint64 * 4)()
        _capi.check(_dev.lib().lmc_sampler_tv_exit_stats(self._h, {"prior": 0, "ncvx": 1}[which], _dev.ptr(passes), rr, _dev.stream_ptr(self.device)))
        return passes, [int(v) for v in rr]

    # -- empirical-Bayes prior weight (SAPG; definition in include/lmc_atomi.h) -----------------
    def set_prior_weight(self, theta):
        """The weight of ``proxg`` (``lmc_problem.prior_sigma``) for every later launch of this sampler: afterwards it runs exactly what a sampler
        created with that weight runs.  MYULA and SK-ROCK; MYMALA, ULPDA, a warm-started TV dual, array-valued ``epsg`` and priors without a
        weight raise ``NotImplementedError``, a weight that is not finite and positive ``ValueError``."""
        _check_sapg(_dev.lib().lmc_sampler_set_prior_sigma(self._h, float(theta)))
        self.prior_weight = float(np.float32(theta))

    def estimate_prior_weight(self, n_updates, theta_bounds, theta0=None, warmup=0, iters_per_update=1, step_scale=10., step_exponent=0.8,
                              average_from=None, dim_eff=None, noise=None):
        """SAPG estimate of the weight of ``proxg`` by marginal maximum likelihood (Vidal, De Bortoli, Pereyra, Durmus 2020, Algorithm 1), on
        the device: ``warmup`` iterations at ``theta0`` (default: the weight of ``proxg``), then ``n_updates`` times { ``iters_per_update``
        iterations, the mean over the chains of the prior value of the new state, one projected step on log theta with step
        ``step_scale (n + 1)^(-step_exponent) / dim_eff`` }, theta kept inside ``theta_bounds = (lo, hi)``.  Returns a :class:`SAPGResult`
        whose ``theta`` is the mean of the iterates after update ``average_from`` (default ``n_updates // 2``); the sampler's weight is that
        mean afterwards.  The moment accumulators take nothing during the call; the iteration counter advances.  ``noise`` (only with
        noise='injected'): ``[warmup + n_updates * iters_per_update, n_chains, H, W]``.  Argument errors raise ``ValueError``, what the
        library has no path for ``NotImplementedError``."""
        if theta0 is None:
            theta0 = _prior_weight(self.proxg)
        cfg = _sapg_config(n_updates, theta_bounds, theta0, warmup, iters_per_update, step_scale, step_exponent, average_from, dim_eff)
        d, k = sapg_dimension(self.proxg, self.dims)
        n_iters = cfg.warmup_iters + cfg.n_updates * cfg.iters_per_update
        nt = None
        if noise is not None:
            nt = _dev.to_dev(noise, self.device)
            if nt.numel() != n_iters * self.n_chains * self.dims[0] * self.dims[1]:
                raise ValueError("noise must have shape [warmup + n_updates * iters_per_update, n_chains, H, W]")
        trace = np.zeros(cfg.n_updates + 1, dtype=np.float64)
        stat = np.zeros(cfg.n_updates, dtype=np.float64)
        bar = C.c_double()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _check_sapg(_dev.lib().lmc_sampler_sapg(self._h, C.byref(cfg), _dev.ptr(nt), dp(trace), dp(stat), C.byref(bar), _dev.stream_ptr(self.device)))
        self.prior_weight = float(np.float32(bar.value))
        return SAPGResult(float(bar.value), trace, stat, float(cfg.dim_eff) if cfg.dim_eff > 0 else d, k)

    # -- diagnostics ---------------------------------------------------------------------
    def energies(self):
        """Per-chain ``f(x_c)``, ``g(x_c)`` (float64 tensors in HBM) -- the energy log of algs.py:578-582."""
        f = torch.empty(self.n_chains, dtype=torch.float64, device=self.device)
        g = torch.empty(self.n_chains, dtype=torch.float64, device=self.device)
        _capi.check(_dev.lib().lmc_sampler_energies(self._h, _dev.ptr(f), _dev.ptr(g), _dev.stream_ptr(self.device)))
        return f, g

    def noise_field(self, iteration):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_sampler_noise(self._h, int(iteration), _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    def _pair(self, shape, fn, *head):
        """Two float64 tensors of ``shape`` and a ``uint64`` count through entry point ``fn(handle, *head, a, b, &count, stream)``."""
        a = torch.empty(shape, dtype=torch.float64, device=self.device)
        b = torch.empty_like(a)
        cnt = C.c_uint64()
        _capi.check(getattr(_dev.lib(), fn)(self._h, *head, _dev.ptr(a), _dev.ptr(b), C.byref(cnt), _dev.stream_ptr(self.device)))
        return a, b, int(cnt.value)

    def moments(self):
        """(sum [H,W] f64, sumsq [H,W] f64, count) over chains and kept iterations."""
        return self._pair(self.dims, "lmc_sampler_get_moments")

    def allreduce_moments(self, rccl_comm):
        """Job-wide (sum, sumsq, count): ONE ``ncclAllReduce`` (RCCL over xGMI) of the packed accumulators through the C ABI
        (``lmc_allreduce_moments``).  ``rccl_comm``: an ``ncclComm_t`` as an integer / ``c_void_p`` (``None`` or 0 = a job of one rank)."""
        return self._pair(self.dims, "lmc_allreduce_moments", _comm(rccl_comm))

    def reset_moments(self):
        _capi.check(_dev.lib().lmc_sampler_reset_moments(self._h, _dev.stream_ptr(self.device)))

    def _block_shape(self, scale):
        s = int(scale)
        return (-(-self.dims[0] // s), -(-self.dims[1] // s))

    def block_moments(self, scale):
        """(S1, S2, count) of one enabled scale: the sums of b and of b^2 over chains and kept iterations, b = the SUM of a sample over
        a ``scale`` x ``scale`` block (``[ceil(H/scale), ceil(W/scale)]`` f64; edge blocks are partial).  :func:`block_mean_var` turns
        them into the mean and the variance of the block mean."""
        return self._pair(self._block_shape(scale), "lmc_sampler_get_block_moments", int(scale))

    def allreduce_block_moments(self, rccl_comm, scale):
        """Job-wide :meth:`block_moments` of one scale: ONE ``ncclAllReduce`` through the C ABI (``lmc_allreduce_block_moments``)."""
        return self._pair(self._block_shape(scale), "lmc_allreduce_block_moments", _comm(rccl_comm), int(scale))

    def _hist_call(self, fn, *head):
        if self.hist_bins is None:
            raise ValueError("the sampler keeps no histogram (hist_bins=, hist_range=)")
        counts = torch.empty((self.hist_bins + 2,) + self.dims, dtype=torch.int64, device=self.device)
        cnt = C.c_uint64()
        _capi.check(getattr(_dev.lib(), fn)(self._h, *head, _dev.ptr(counts), C.byref(cnt), _dev.stream_ptr(self.device)))
        return counts, int(cnt.value)

    def histogram(self):
        """(counts ``[hist_bins + 2, H, W]`` ``torch.int64``, count): the pixel histogram over chains and kept iterations.  Row 0 counts the
        samples below ``lo``, row ``1 + k`` those of bin ``k``, the last row everything at or above ``hi`` (NaN included); the rows of a pixel
        sum to ``count``."""
        return self._hist_call("lmc_sampler_get_histogram")

    def allreduce_histogram(self, rccl_comm):
        """Job-wide :meth:`histogram`: ONE ``ncclAllReduce`` of the integer counters through the C ABI (``lmc_allreduce_histogram``)."""
        return self._hist_call("lmc_allreduce_histogram", _comm(rccl_comm))

    def _group_call(self, fn, *head):
        if self.chain_groups is None:
            raise ValueError("the sampler keeps no chain-group moments (chain_groups=)")
        S1 = torch.empty((self.chain_groups,) + self.dims, dtype=torch.float64, device=self.device)
        S2 = torch.empty_like(S1)
        cnt = (C.c_uint64 * self.chain_groups)()
        _capi.check(getattr(_dev.lib(), fn)(self._h, *head, _dev.ptr(S1), _dev.ptr(S2), cnt, _dev.stream_ptr(self.device)))
        return S1, S2, torch.tensor([int(v) for v in cnt], dtype=torch.int64)

    def group_moments(self):
        """(S1, S2 ``[chain_groups, H, W]`` f64, counts ``[chain_groups]`` int64 CPU tensor): the sums of x and x^2 over the kept samples of every
        chain group (global chain id mod ``chain_groups``) and the samples per group.  :func:`mcse_from_group_moments` turns them into the
        Monte-Carlo error of the mean and the variance and the effective sample size, per pixel."""
        return self._group_call("lmc_sampler_get_group_moments")

    def allreduce_group_moments(self, rccl_comm):
        """Job-wide :meth:`group_moments`: ONE ``ncclAllReduce`` of the packed sums and counts through the C ABI (``lmc_allreduce_group_moments``)."""
        return self._group_call("lmc_allreduce_group_moments", _comm(rccl_comm))

    def cov_sketch(self):
        """(Y ``[k, H, W]``, s ``[k]``, Q ``[k, k]`` f64, n): the sums of the covariance sketch over the kept samples (``cov_probes=``) and the number
        of samples, which is the count of :meth:`moments`.  :func:`cov_from_sketch` turns them, with ``moments()[0]`` and ``cov_center``, into
        covariances."""
        if self.cov_k is None:
            raise ValueError("the sampler keeps no covariance sketch (cov_probes=)")
        k = self.cov_k
        Y = torch.empty((k,) + self.dims, dtype=torch.float64, device=self.device)
        sv = torch.empty(k, dtype=torch.float64, device=self.device)
        Q = torch.empty((k, k), dtype=torch.float64, device=self.device)
        cnt = C.c_uint64()
        _capi.check(_dev.lib().lmc_sampler_get_cov_sketch(self._h, _dev.ptr(Y), _dev.ptr(sv), _dev.ptr(Q), C.byref(cnt), _dev.stream_ptr(self.device)))
        return Y, sv, Q, int(cnt.value)


class ULPDASampler(MYULASampler):
    """Many-chain ULPDA on one GPU (algs.py:425-449).  ``proxf`` = data term (L2 with Convolve2D / Diagonal / Identity /
    no operator), ``proxg`` = L21 (isotropic) or L1 (anisotropic) acting on ``A x`` with ``A`` the forward-difference
    gradient.  The implicit data step runs ``proxf.niter`` warm-started CG iterations per chain on the GPU."""

    def __init__(self, proxf, proxg, A, dims, n_chains=1, tau=None, mu=None, theta=1.0, gfirst=True, z=None, seed=0,
                 chain_offset=0, noise="philox", moments=False, burn_in=0, thin=1, device=None, variant=None, implicit_tol=None,
                 moment_scales=None, hist_bins=None, hist_range=None, chain_groups=None, cov_probes=None, cov_center=None):
        from .operators import Gradient
        from .proximal import L1, L21
        acc = _check_accumulators(locals(), moments, dims)      # before anything touches the proxes
        if not isinstance(A, Gradient):
            raise NotImplementedError("ULPDA on the GPU supports A = Gradient (the reference's operator, prox_lmc_deconv.py:98)")
        if getattr(proxg, "bounds", None) is not None:
            raise NotImplementedError("ULPDA does not take a prior with bounds: its prior enters through the dual ball of g o A, which has no box form; use MYULA")
        _refuse_radon(_data_descriptor(proxf), {}, {}, ("ULPDA", "its primal step is the implicit step of f, which is not built for the Radon operator; use MYULA"))
        _refuse_sense(_data_descriptor(proxf), {}, {}, ("ULPDA", "its primal step is the implicit step of f, which is diagonal in neither the pixel nor the Fourier basis for coil maps; use MYULA"))
        _refuse_term(_data_descriptor(proxf), {}, {}, {
            "poisson": ("ULPDA", "its primal step is the implicit step of f, which has no closed form for the Poisson likelihood; use MYULA"),
            "wl2": ("ULPDA", "its primal step is the implicit step of f, (I + tau sigma Op^T W Op)^{-1}, which is not built; use MYULA"),
            "huber": ("ULPDA", "its primal step is the implicit step of f, which is not built for the Huber loss under an operator; use MYULA")})
        _refuse_spectral(_data_descriptor(proxf), {}, {}, ("ULPDA", "its primal-dual loop is not wired to the closed-form implicit step of this term; use MYULA"))
        _refuse_psf(_data_descriptor(proxf), {}, {}, ("ULPDA", "its primal step is the implicit step of f, which is not built for a large PSF; use MYULA"))
        if isinstance(proxg, L21):
            prior = {"prior_kind": _capi.PRIOR_TV_ISO, "prior_sigma": proxg.sigma, "tv_niter": 1, "tv_betas": [0.0]}
        elif isinstance(proxg, L1):
            prior = {"prior_kind": _capi.PRIOR_TV_ANISO, "prior_sigma": proxg.sigma}
        else:
            raise NotImplementedError(f"{type(proxg).__name__} has no dual-prox device functor (L21 or L1 expected)")
        self.dims = (int(dims[0]), int(dims[1]))
        self.n_chains = int(n_chains)
        self.device = _dev.device(device)
        self.proxf, self.proxg = proxf, proxg
        # implicit_tol: relative residual of THIS sampler's implicit data step (None = the library default, set_cg_tolerance;
        # 0 or negative = disabled: always all iterations)
        tol = 0.0 if implicit_tol is None else (float(implicit_tol) if implicit_tol > 0 else -1.0)
        self._problem = _Problem(self.dims, _data_descriptor(proxf), prior, self.device,
                                 options={"step_variant": variant or 0, "implicit_tol": tol})
        cfg = _capi.lmc_ulpda_config()
        cfg.struct_size = C.sizeof(_capi.lmc_ulpda_config)
        cfg.problem = self._problem.c
        cfg.n_chains = self.n_chains
        cfg.chain_offset = int(chain_offset)
        cfg.tau, cfg.mu, cfg.theta = float(tau), float(mu), float(theta)
        cfg.gfirst = 1 if gfirst else 0
        cfg.cg_niter = int(getattr(proxf, "niter", 10) or 10)
        cfg.warm = 1 if getattr(proxf, "warm", True) else 0
        self._z = None
        if z is not None:
            self._z = _dev.to_dev(z, self.device).reshape(self.dims)
            cfg.z_dev = self._z.data_ptr()
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.noise_mode = {"philox": _capi.NOISE_PHILOX, "injected": _capi.NOISE_INJECTED, "none": _capi.NOISE_NONE}[noise]
        cfg.moments = 1 if moments else 0
        cfg.burn_in = int(burn_in)
        cfg.thin = int(thin)
        self.noise_mode = noise
        self.moments_on = bool(moments)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _capi.check(_dev.lib().lmc_ulpda_create(C.byref(cfg), C.byref(self._h)))
        self._attach_accumulators(acc)

    def set_steps(self, tau, mu):
        _capi.check(_dev.lib().lmc_sampler_set_steps(self._h, float(tau), float(mu)))

    def set_dual(self, y):
        yt = _dev.to_dev(y, self.device)
        n2 = 2 * self.dims[0] * self.dims[1]
        if yt.numel() == n2:
            yt = yt.reshape(1, n2).expand(self.n_chains, n2).contiguous()
        if yt.numel() != self.n_chains * n2:
            raise ValueError("dual state must have 2*H*W entries per chain")
        _capi.check(_dev.lib().lmc_sampler_set_dual(self._h, _dev.ptr(yt), _dev.stream_ptr(self.device)))
        torch.cuda.current_stream(self.device).synchronize()

    def get_dual(self):
        out = torch.empty((self.n_chains, 2) + self.dims, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_sampler_get_dual(self._h, _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out


def UnadjustedLangevinPrimalDual(proxf, proxg, A, x0, tau, mu, y0=None, z=None, theta=1., niter=10, seed=0, gfirst=True,
                                 callback=None, callbacky=False, returny=False, show=False, *, n_chains=None, dims=None,
                                 rng="philox", chain_offset=0, burn_in=0, thin=1, device=None, diagnostics=None, moment_scales=None,
                                 hist_bins=None, hist_range=None, quantiles=(0.05, 0.5, 0.95), chain_groups=None, cov_probes=None, cov_center=None):
    r"""Unadjusted Langevin Primal-Dual algorithm (ULPDA) -- drop-in for algs.py:295-474.

    Reference form (``n_chains is None``): one chain, returns ``np.ndarray (niter, n)`` (and the duals ``(niter, 2n)`` with
    ``returny``), ``callback(x)`` / ``callback(x, y)`` every iteration, ``tau`` / ``mu`` scalars or per-iteration arrays
    (algs.py:402-408).  ``rng='pcg64'`` injects the reference's noise stream.  Many-chain form: :class:`MYULAResult`
    (``diagnostics=(ph, pw)`` or ``True``: split R-hat / ESS across chains as in :func:`MoreauYosidaUnadjustedLangevin`;
    ``moment_scales``, ``hist_bins`` / ``hist_range`` / ``quantiles``, ``chain_groups``, ``cov_probes`` / ``cov_center``: as there).
    """
    dims = _dims_of(dims, A, proxf)
    many = n_chains is not None
    C_ = int(n_chains) if many else 1
    n = int(dims[0]) * int(dims[1])
    if rng not in ("philox", "pcg64"):
        raise ValueError("rng must be 'philox' or 'pcg64'")
    if rng == "pcg64" and C_ != 1:
        raise ValueError("rng='pcg64' reproduces the reference's single chain; use n_chains=None")
    acc = _accumulator_keywords(locals(), many, C_, dims)
    taus = np.full(niter, tau, dtype=np.float64) if np.isscalar(tau) else np.asarray(tau, dtype=np.float64)
    mus = np.full(niter, mu, dtype=np.float64) if np.isscalar(mu) else np.asarray(mu, dtype=np.float64)
    smp = ULPDASampler(proxf, proxg, A, dims, n_chains=C_, tau=taus[0], mu=mus[0], theta=theta, gfirst=gfirst, z=z,
                       seed=seed, chain_offset=chain_offset, noise="injected" if rng == "pcg64" else "philox",
                       moments=many, burn_in=burn_in, thin=thin, device=device, **acc)
    with smp:
        smp.set_state(x0)
        if y0 is not None:
            smp.set_dual(y0)
        tstart = time.time()
        if show:
            print('Unadjusted Langevin primal-dual (lmc_atomi_amd / HIP): U(x) = f(x) + x^T z + g(Ax)\n'
                  '---------------------------------------------------------\n'
                  'Proximal operator (f): %s\nProximal operator (g): %s\nLinear operator (A): %s\n'
                  'tau = %s\t\tmu = %s\ntheta = %.2f\t\tniter = %d\tchains = %d\n' %
                  (type(proxf), type(proxg), type(A), str(taus[0]), str(mus[0]), theta, niter, C_))
            print('   Itn       x[0]          f         g o A      U = f + g o A')
        host_rng = default_rng(seed) if rng == "pcg64" else None
        xs = np.empty((niter, n), dtype=np.float64) if not many else None
        ys = np.empty((niter, 2 * n), dtype=np.float64) if (returny and not many) else None
        tracer = None
        if diagnostics and many:
            from .diagnostics import ChainTrace
            tracer = ChainTrace(smp, (8, 8) if diagnostics is True else diagnostics)
        for it in range(niter):
            smp.set_steps(taus[it], mus[it])
            if host_rng is not None:
                xi = host_rng.standard_normal(n)                        # algs.py:433
                smp.step(1, noise=xi.reshape(1, 1, *smp.dims))
            else:
                smp.step(1)
            if not many:
                xs[it] = smp.get_state().reshape(-1).cpu().numpy()
                if returny or callbacky:
                    yk = smp.get_dual().reshape(-1).cpu().numpy()
                    if returny:
                        ys[it] = yk
                if callback is not None:
                    callback(xs[it], yk) if callbacky else callback(xs[it])
            elif callback is not None:
                callback(smp.get_state(), smp.get_dual()) if callbacky else callback(smp.get_state())
            if tracer is not None and it >= burn_in and (it - burn_in) % thin == 0:      # the iterations that enter the moments
                tracer.record()
            if show and (it < 10 or niter - it < 10 or it % max(niter // 10, 1) == 0):
                f, g = smp.energies()
                x00 = float(smp.get_state().reshape(-1)[0])
                print('%6g  %12.5e  %10.3e  %10.3e      %10.3e' % (it + 1, x00, float(f.mean()), float(g.mean()),
                                                                  float((f + g).mean())))
        if show:
            print('\nTotal time (s) = %.2f' % (time.time() - tstart))
            print('---------------------------------------------------------\n')
        if not many:
            return (xs, ys) if returny else xs
        return _result(smp, quantiles, tstart, tracer)


class MYULAResult:
    """Return value of the many-chain form of :func:`MoreauYosidaUnadjustedLangevin`."""

    def __init__(self, state, mean, var, count, energy_f, energy_g, elapsed, diagnostics=None, trace=None, scale_mean=None, scale_std=None, hist=None, groups=None, cov=None):
        self.state, self.mean, self.var, self.count = state, mean, var, count
        # chain_groups: Monte-Carlo standard error of mean and var and the effective sample size, [H, W] float64 each (mcse_from_group_moments), and the
        # samples per chain group [G] int64; None when not asked
        self.mcse_mean, self.mcse_var, self.ess, self.group_counts = groups if groups is not None else (None, None, None, None)
        # cov_probes: the covariances of the sketch (CovSketch: cov_xt, cov_tt, t_mean, n; cov_from_sketch); None when not asked
        self.cov_sketch = cov
        # hist_bins / hist_range: the pixel histogram [B + 2, H, W] int64 with its lo and scale (None when not asked), and {q: tensor [H, W]} of
        # the quantiles asked for (hist_quantiles; empty without a histogram)
        self.hist, self.hist_lo, self.hist_scale, self.quantiles = hist if hist is not None else (None, None, None, {})
        # moment_scales: posterior mean and standard deviation of the image averaged over s x s blocks, {s: tensor [ceil(H/s), ceil(W/s)]}; empty when not asked
        self.scale_mean, self.scale_std = dict(scale_mean or {}), dict(scale_std or {})
        self.energy_f, self.energy_g, self.elapsed = energy_f, energy_g, elapsed
        self.diagnostics, self.trace = diagnostics, trace      # split R-hat / ESS across chains (diagnostics.py), [T, C, Q] trace


def _result(smp, quantiles, tstart, tracer=None):
    """The :class:`MYULAResult` of a sampler that has finished its iterations (``tracer``: the :class:`ChainTrace` of a run with diagnostics)."""
    s1, s2, cnt = smp.moments()
    f, g = smp.energies()
    state = smp.get_state()
    torch.cuda.current_stream().synchronize()
    mean, var = mean_var_from_moments(s1, s2, max(cnt, 1))
    scale_mean, scale_std = _scale_summaries(smp)
    diag = tracer.summary() if tracer is not None and len(tracer) else None
    return MYULAResult(state, mean, var, cnt, f, g, time.time() - tstart, diagnostics=diag,
                       trace=tracer.trace() if diag is not None else None, scale_mean=scale_mean, scale_std=scale_std,
                       hist=_hist_summaries(smp, quantiles), groups=_group_summaries(smp), cov=_cov_summary(smp, s1))


def _run(smp, x0, niter, callback):
    """``niter`` iterations of a many-chain sampler from ``x0``: one ``step`` call, or step and ``callback(state)``.  Returns the start time."""
    smp.set_state(x0)
    tstart = time.time()
    if callback is None:
        smp.step(niter)
    else:
        for _ in range(niter):
            smp.step(1)
            callback(smp.get_state())
    return tstart


def MoreauYosidaUnadjustedLangevin(proxf, proxg, x0, tau=None, gamma=.1, epsg=1., niter=10, seed=0,
                                   callback=None, show=False, *, n_chains=None, dims=None, rng="philox",
                                   chain_offset=0, burn_in=0, thin=1, device=None, diagnostics=None, moment_scales=None,
                                   hist_bins=None, hist_range=None, quantiles=(0.05, 0.5, 0.95), chain_groups=None, cov_probes=None, cov_center=None):
    r"""Moreau--Yosida Unadjusted Langevin algorithm (MYULA) -- drop-in for algs.py:477-587.

    .. math::
        x^{k+1} = (1-\tau/\gamma)x^k - \tau\nabla f(x^k) + (\tau/\gamma)\,prox_{\gamma\epsilon g}(x^k)
                  + \sqrt{2\tau}\,\xi^k

    Reference form (``n_chains is None``): one chain, returns ``np.ndarray (niter, n)`` holding
    every iterate, ``callback(x)`` after every iteration, ``show`` prints the reference's log.
    ``rng='pcg64'`` draws the noise exactly as the reference does (``default_rng(seed)``, one
    ``standard_normal(n)`` per iteration, algs.py:561,565) and injects it, so the trajectory
    equals the reference's to fp32 rounding; ``rng='philox'`` (default) draws on the GPU.

    Many-chain form (``n_chains=C``): runs C chains from ``x0`` (one image or ``[C,H,W]``), keeps
    no iterates, returns a :class:`MYULAResult` (final states, posterior mean / variance over
    chains and kept iterations, per-chain energies).  ``diagnostics=(ph, pw)`` (or ``True`` = (8, 8)) additionally records,
    at every kept iteration, a ph x pw grid of block means and the energies of every chain and returns split R-hat and
    effective sample size across chains in ``result.diagnostics`` (:mod:`lmc_atomi_amd.diagnostics`).  ``moment_scales=(2, 4, 8, 16)`` (any
    subset) additionally returns the posterior mean and standard deviation of the image averaged over s x s blocks -- uncertainty at
    several scales -- in ``result.scale_mean[s]`` / ``result.scale_std[s]``.  ``hist_bins=B`` (1 .. 62) with ``hist_range=(lo, hi)`` (scalars or
    ``[H, W]`` arrays, e.g. mean -+ 5 std of a pilot run) keeps a histogram per pixel over the kept samples: ``result.hist`` (counters
    ``[B + 2, H, W]``), ``result.hist_lo`` / ``result.hist_scale``, and the pixel-wise quantile maps ``result.quantiles[q]`` for every ``q`` in
    ``quantiles`` -- credible intervals that, unlike mean -+ 2 std, follow the skew of a TV posterior next to edges (:func:`hist_quantiles`,
    :func:`hist_exceedance`).  ``chain_groups=G`` (2 .. 64, at most ``n_chains``) splits the chains into G groups by global chain id mod G and returns the
    pixel-wise Monte-Carlo standard errors ``result.mcse_mean`` and ``result.mcse_var`` of ``result.mean`` and ``result.var``, the effective sample size
    ``result.ess`` and the samples per group ``result.group_counts`` (:func:`mcse_from_group_moments`: the scatter of the group means, which includes
    the autocorrelation of the chains; one pixel of these maps is precise to sqrt(2 / (G - 1)), 25 % at G = 32).
    ``cov_probes=P`` (``[k, H, W]``, k <= 32; region indicators, or :func:`random_probes`) with ``cov_center=m`` (``[H, W]``, best the mean of a pilot run;
    None = 0, which costs digits) keeps the covariance sketch of the kept samples and returns ``result.cov_sketch``, a :class:`CovSketch`: ``cov_xt[j]`` the
    covariance of every pixel with the projection on probe j, ``cov_tt`` the covariance matrix of the projections (of the region fluxes), ``.corr(result.var)``
    the correlation maps and ``.modes(r)`` the leading eigenvalues and eigen-images of the Nystrom approximation of the posterior covariance (exact when its
    rank is at most k, lower bounds otherwise).
    """
    if isinstance(proxg, VectorialTV):
        # multi-channel images: the sampler of its own, many-chain form only (n_chains=None: one chain); x0 [nch, H, W] or [nch, C, H, W]
        asked = {"moment_scales": moment_scales, "hist_bins": hist_bins, "hist_range": hist_range, "chain_groups": chain_groups, "cov_probes": cov_probes,
                 "cov_center": cov_center, "callback": callback, "diagnostics": diagnostics or None,
                 "quantiles": None if quantiles is None or tuple(quantiles) == (0.05, 0.5, 0.95) else quantiles,
                 "show": show or None, "rng='pcg64'": None if rng == "philox" else rng}
        for name, value in asked.items():
            if value is not None:
                raise NotImplementedError(f"{name} is not built for multi-channel images (VectorialTV): the multi-channel sampler keeps the pixel moments "
                                          "and the energies only")
        return _multichannel_myula(proxf, proxg, x0, tau, gamma, epsg, niter, seed, n_chains, dims, chain_offset, burn_in, thin, device)
    dims = _dims_of(dims, proxf, proxg)
    many = n_chains is not None
    C_ = int(n_chains) if many else 1
    n = int(dims[0]) * int(dims[1])
    if rng not in ("philox", "pcg64"):
        raise ValueError("rng must be 'philox' or 'pcg64'")
    if rng == "pcg64" and C_ != 1:
        raise ValueError("rng='pcg64' reproduces the reference's single chain; use n_chains=None")
    acc = _accumulator_keywords(locals(), many, C_, dims)
    smp = MYULASampler(proxf, proxg, dims, n_chains=C_, tau=tau, gamma=gamma, epsg=epsg, seed=seed,
                       chain_offset=chain_offset, noise="injected" if rng == "pcg64" else "philox",
                       moments=many, burn_in=burn_in, thin=thin, device=device, **acc)
    with smp:
        smp.set_state(x0)
        tstart = time.time()
        if show:
            print('Moreau--Yosida Unadjusted Langevin (lmc_atomi_amd / HIP)\n'
                  '---------------------------------------------------------\n'
                  'Proximal operator (f): %s\nProximal operator (g): %s\n'
                  'tau = %s\tgamma=%10e\nepsg = %s\tniter = %d\tchains = %d\n' %
                  (type(proxf), type(proxg), str(tau), gamma, str(epsg) if np.asarray(epsg).size == 1 else 'Multi', niter, C_))     # algs.py:539-542
            print('   Itn       x[0]          f           g     J = f + eps*g')
        if not many:
            samples = np.empty((niter, n), dtype=np.asarray(x0).dtype if not isinstance(x0, torch.Tensor) else np.float32)
            host_rng = default_rng(seed) if rng == "pcg64" else None
            buf = torch.empty(smp.shape, dtype=torch.float32, device=smp.device)
            for it in range(niter):
                if host_rng is not None:
                    xi = host_rng.standard_normal(n)                  # algs.py:565
                    smp.step(1, noise=xi.reshape(1, 1, *smp.dims))
                else:
                    smp.step(1)
                smp.get_state(buf)
                xk = buf.reshape(-1).cpu().numpy()
                samples[it] = xk
                if callback is not None:
                    callback(samples[it])
                if show and (it < 10 or niter - it < 10 or it % max(niter // 10, 1) == 0):
                    f, g = smp.energies()
                    pf, pg = float(f[0]), float(g[0])
                    print('%6g  %12.5e  %10.3e  %10.3e  %10.3e' % (it + 1, samples[it][0], pf, pg, pf + float(np.sum(epsg * pg))))   # algs.py:582
            if show:
                print('\nTotal time (s) = %.2f' % (time.time() - tstart))
                print('---------------------------------------------------------\n')
            return samples
        # many chains: no iterates kept
        tracer = None
        if diagnostics:
            from .diagnostics import ChainTrace
            tracer = ChainTrace(smp, (8, 8) if diagnostics is True else diagnostics)
        next_rec = burn_in + 1                       # iteration counts after which the sampler has accumulated moments
        done = 0
        while done < niter:
            chunk = niter - done if (callback is None and not show) else 1
            if tracer is not None and next_rec > done:
                chunk = min(chunk, next_rec - done)
            smp.step(chunk)
            done += chunk
            if tracer is not None and done == next_rec:
                tracer.record()
                next_rec += thin
            if callback is not None:
                callback(smp.get_state())
            if show and (done <= 10 or niter - done < 10 or (done - 1) % max(niter // 10, 1) == 0):
                f, g = smp.energies()
                x00 = float(smp.get_state()[0, 0, 0])
                print('%6g  %12.5e  %10.3e  %10.3e  %10.3e' % (done, x00, float(f.mean()), float(g.mean()),
                                                              float((f + (epsg if np.asarray(epsg).size == 1 else float(np.sum(epsg))) * g).mean())))
        return _result(smp, quantiles, tstart, tracer)


def _multichannel_data(proxf, n_channels, dims):
    """The per-channel data terms of a multi-channel sampler as one description: ``(data descriptor of channel 0 without y and mask, y [nch, H, W] or None,
    masks [nch, H, W] or None)``.  Host checks only, before any device call: a sequence of ``n_channels`` :class:`L2` terms with the same operator kind
    (``Convolve2D``, ``Diagonal``, ``Identity`` or none), the same taps and offset and the same ``sigma``; ``None`` = no data term."""
    if proxf is None:
        return {"data_kind": _capi.DATA_NONE}, None, None
    try:
        terms = list(proxf)
    except TypeError:
        raise ValueError(f"proxf must be a sequence of {n_channels} L2 terms, one per channel (got {type(proxf).__name__})") from None
    if len(terms) != n_channels:
        raise ValueError(f"proxf holds {len(terms)} terms for {n_channels} channels: one L2 term per channel")
    n = int(dims[0]) * int(dims[1])
    for t in terms:
        if not isinstance(t, L2):
            raise NotImplementedError(f"the multi-channel sampler is built for L2 data terms per channel; {type(t).__name__} (Poisson, Huber, ...) is not built")
        if t.weights is not None or getattr(t, "_spectral", None) is not None:
            raise ValueError("the multi-channel sampler takes unweighted L2 terms: per-pixel weights are not built per channel")
        if t.Op is not None and not isinstance(t.Op, (Convolve2D, Diagonal, Identity)):
            raise NotImplementedError(f"the multi-channel sampler is built for Op = Convolve2D, Diagonal, Identity or None; {type(t.Op).__name__} is not built per channel")
        if t.b is None:
            raise ValueError("every channel's L2 term needs its observation b")
        if np.size(t.b) != n:
            raise ValueError(f"a channel's b has {np.size(t.b)} entries for an image of shape {tuple(dims)}")
    kind = lambda t: Identity if t.Op is None else type(t.Op)
    if any(kind(t) is not kind(terms[0]) for t in terms):
        raise ValueError("the channels' L2 terms must have the same operator kind (Convolve2D, Diagonal, Identity or none)")
    if any(float(t.sigma) != float(terms[0].sigma) for t in terms):
        raise ValueError("the channels' L2 terms must have the same sigma: sigma_f is shared by the channels")
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    y = np.stack([host(t.b).astype(np.float32).reshape(dims) for t in terms])
    data, masks = {"sigma_f": float(terms[0].sigma)}, None
    op = terms[0].Op
    if isinstance(op, Convolve2D):
        for t in terms[1:]:
            if np.shape(t.Op.h) != np.shape(op.h) or not np.array_equal(np.asarray(t.Op.h), np.asarray(op.h)) or tuple(t.Op.offset) != tuple(op.offset):
                raise ValueError("the channels' blurs must have the same taps and offset: the blur is shared by the channels")
        data.update(data_kind=_capi.DATA_BLUR, h=op.h, offset=op.offset)
    elif isinstance(op, Diagonal):
        for t in terms:
            if np.size(t.Op.d) != n:
                raise ValueError(f"a channel's mask has {np.size(t.Op.d)} entries for an image of shape {tuple(dims)}")
        masks = np.stack([host(t.Op.d).astype(np.float32).reshape(dims) for t in terms])
        data["data_kind"] = _capi.DATA_MASK
    else:
        data["data_kind"] = _capi.DATA_IDENTITY
    return data, y, masks


class MultichannelMYULASampler:
    """Many-chain MYULA on multi-channel images under the vectorial TV prior: owns an ``lmc_mch`` handle (include/lmc_atomi.h).

    ``proxf``: a sequence of ``n_channels`` :class:`L2` terms, one per channel -- each channel has its own ``b`` and, with ``Op = Diagonal``, its own mask (a
    Bayer mosaic); the operator kind (``Convolve2D``, ``Diagonal``, ``Identity`` or none), the taps and offset and ``sigma`` are shared (a mismatch, or
    weights: ``ValueError``; any other term: ``NotImplementedError``).  ``proxg``: a :class:`VectorialTV` of that many channels.
    State in HBM: ``[n_channels, n_chains, H, W]`` fp32, channel-major.  Channel ``ch`` draws the Philox field of the seed ``(seed + (ch << 32)) mod 2^64``:
    channel 0 is the field of :class:`MYULASampler` with the same seed, and any sharding of the chains reproduces the same trajectories.
    One iteration: the coupled prox over all chains and channels, then per channel the fused step kernel with that prox as a ready-made one."""

    def __init__(self, proxf, proxg, dims, n_chains=1, tau=None, gamma=0.1, epsg=1.0, seed=0, chain_offset=0, noise="philox", moments=False,
                 burn_in=0, thin=1, device=None, variant=None):
        if not isinstance(proxg, VectorialTV):
            raise NotImplementedError(f"MultichannelMYULASampler is built for proxg = VectorialTV (got {type(proxg).__name__}); single-plane priors run in MYULASampler")
        if tau is None:
            raise NotImplementedError("tau=None (backtracking) is not implemented by the reference loop either")
        if np.asarray(epsg).size > 1:
            raise NotImplementedError("array-valued epsg is built for the closed-form priors only: VectorialTV takes a scalar epsg")
        self.dims = (int(dims[0]), int(dims[1]))
        if self.dims != proxg.dims:
            raise ValueError(f"dims {self.dims} differ from the prior's {proxg.dims}")
        self.n_channels = proxg.n_channels
        data, y, masks = _multichannel_data(proxf, self.n_channels, self.dims)
        if noise not in ("philox", "injected", "none"):
            raise ValueError("noise must be 'philox', 'injected' or 'none'")
        self.n_chains = int(n_chains)
        self.device = _dev.device(device)
        self.proxf, self.proxg = proxf, proxg
        self._problem = _Problem(self.dims, data, proxg.prior_descriptor(), self.device, options={"step_variant": variant or 0, "multichannel": True})
        cfg = _capi.lmc_mch_config()
        cfg.struct_size = C.sizeof(_capi.lmc_mch_config)
        cfg.problem = self._problem.c
        self._y = self._masks = None
        if y is not None:
            self._y = _dev.to_dev(y, self.device)
            cfg.problem.y_dev = self._y.data_ptr()
        shared = masks is not None and all(np.array_equal(masks[0], m) for m in masks[1:])
        if masks is not None:
            self._masks = _dev.to_dev(masks[0] if shared else masks, self.device)
            cfg.problem.mask_dev = self._masks.data_ptr()
            cfg.mask_channel_stride = 0 if shared else self.dims[0] * self.dims[1]
        cfg.n_channels = self.n_channels
        cfg.n_chains = self.n_chains
        cfg.chain_offset = int(chain_offset)
        cfg.tau, cfg.gamma, cfg.epsg = float(tau), float(gamma), float(epsg)
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.noise_mode = {"philox": _capi.NOISE_PHILOX, "injected": _capi.NOISE_INJECTED, "none": _capi.NOISE_NONE}[noise]
        cfg.moments = 1 if moments else 0
        cfg.burn_in = int(burn_in)
        cfg.thin = int(thin)
        self.noise_mode = noise
        self.moments_on = bool(moments)
        self._h = C.c_void_p()
        torch.cuda.current_stream(self.device).synchronize()      # y and the masks are on the device before the handle reads them
        with torch.cuda.device(self.device):
            _capi.check(_dev.lib().lmc_mch_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _dev.lib().lmc_mch_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def shape(self):
        return (self.n_channels, self.n_chains) + self.dims

    def set_state(self, x):
        """``x``: ``[n_channels, H, W]`` (broadcast to every chain) or ``[n_channels, n_chains, H, W]``."""
        xt = _dev.to_dev(x, self.device)
        n = self.dims[0] * self.dims[1]
        if xt.numel() == self.n_channels * n:
            xt = xt.reshape(self.n_channels, 1, *self.dims).expand(self.shape).contiguous()
        if xt.numel() != self.n_channels * self.n_chains * n:
            raise ValueError(f"state of shape {tuple(xt.shape)} does not match {self.shape}")
        _capi.check(_dev.lib().lmc_mch_set_state(self._h, _dev.ptr(xt), _dev.stream_ptr(self.device)))
        torch.cuda.current_stream(self.device).synchronize()  # xt may be a temporary

    def get_state(self, out=None):
        if out is None:
            out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_mch_get_state(self._h, _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    @property
    def iteration(self):
        return int(_dev.lib().lmc_mch_iteration(self._h))

    @iteration.setter
    def iteration(self, it):
        _capi.check(_dev.lib().lmc_mch_set_iteration(self._h, int(it)))

    def step(self, n_iters=1, noise=None):
        """Run ``n_iters`` iterations on every chain and channel.  ``noise`` (only with noise='injected'): ``[n_iters, n_channels, n_chains, H, W]``."""
        nt = None
        if noise is not None:
            nt = _dev.to_dev(noise, self.device)
            if nt.numel() != n_iters * int(np.prod(self.shape)):
                raise ValueError("noise must have shape [n_iters, n_channels, n_chains, H, W]")
        _capi.check(_dev.lib().lmc_mch_step(self._h, int(n_iters), _dev.ptr(nt), _dev.stream_ptr(self.device)))
        if nt is not None:
            torch.cuda.current_stream(self.device).synchronize()

    @property
    def kernel_name(self):
        return _dev.lib().lmc_mch_kernel_name(self._h).decode()

    def energies(self):
        """Per-chain ``f(x_c) = sum_ch f_ch`` and ``g(x_c) = sigma VTV(x_c)`` (float64 tensors in HBM)."""
        f = torch.empty(self.n_chains, dtype=torch.float64, device=self.device)
        g = torch.empty(self.n_chains, dtype=torch.float64, device=self.device)
        _capi.check(_dev.lib().lmc_mch_energies(self._h, _dev.ptr(f), _dev.ptr(g), _dev.stream_ptr(self.device)))
        return f, g

    def noise_field(self, iteration):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_mch_noise(self._h, int(iteration), _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    def moments(self):
        """(sum [nch, H, W] f64, sumsq [nch, H, W] f64, count) over chains and kept iterations."""
        a = torch.empty((self.n_channels,) + self.dims, dtype=torch.float64, device=self.device)
        b = torch.empty_like(a)
        cnt = C.c_uint64()
        _capi.check(_dev.lib().lmc_mch_get_moments(self._h, _dev.ptr(a), _dev.ptr(b), C.byref(cnt), _dev.stream_ptr(self.device)))
        return a, b, int(cnt.value)

    def reset_moments(self):
        _capi.check(_dev.lib().lmc_mch_reset_moments(self._h, _dev.stream_ptr(self.device)))


def _multichannel_myula(proxf, proxg, x0, tau, gamma, epsg, niter, seed, n_chains, dims, chain_offset, burn_in, thin, device):
    """The many-chain form of :func:`MoreauYosidaUnadjustedLangevin` under a :class:`VectorialTV` prior: ``mean`` / ``var`` ``[nch, H, W]``, ``state``
    ``[nch, C, H, W]``."""
    smp = MultichannelMYULASampler(proxf, proxg, dims if dims is not None else proxg.dims, n_chains=1 if n_chains is None else int(n_chains), tau=tau,
                                   gamma=gamma, epsg=epsg, seed=seed, chain_offset=chain_offset, moments=True, burn_in=burn_in, thin=thin, device=device)
    with smp:
        smp.set_state(x0)
        tstart = time.time()
        smp.step(niter)
        s1, s2, cnt = smp.moments()
        f, g = smp.energies()
        state = smp.get_state()
        torch.cuda.current_stream(smp.device).synchronize()
        mean, var = mean_var_from_moments(s1, s2, max(cnt, 1))
        return MYULAResult(state, mean, var, cnt, f, g, time.time() - tstart)


def sgs_step_bound(rho, gamma):
    """``1 / (1 / rho^2 + 1 / gamma)``: the reciprocal of the Lipschitz constant of the smooth part of the z-potential of the split Gibbs sampler,
    ``||z - x||^2 / (2 rho^2)`` plus the Moreau envelope of ``epsg g`` at ``gamma``.  ``tau`` at or below it is the recommended range of
    :class:`SplitGibbsSampler` (the x-step is an exact draw and bounds nothing).  Host arithmetic, no GPU."""
    rho, gamma = float(rho), float(gamma)
    if not (np.isfinite(rho) and rho > 0 and np.isfinite(gamma) and gamma > 0):
        raise ValueError(f"rho and gamma must be finite and > 0 (got {rho!r}, {gamma!r})")
    return 1.0 / (1.0 / rho ** 2 + 1.0 / gamma)


def _refuse_sgs(data, prior, proxg, epsg):
    """``NotImplementedError`` for what ``lmc_sgs_create`` refuses with ``LMC_E_UNSUPPORTED`` (include/lmc_atomi.h), before a handle exists."""
    who = "the split Gibbs sampler"
    _refuse_vtv(proxg, "SplitGibbsSampler")
    kind = data.get("data_kind")
    blurs = (_capi.DATA_BLUR, _capi.DATA_POISSON_BLUR, _capi.DATA_WL2_BLUR, _capi.DATA_HUBER_BLUR)
    if kind in blurs or kind in _capi.PSF_KINDS:
        raise NotImplementedError(f"{who} draws x | z exactly where the Hessian of the data term is diagonal in the pixel or the Fourier basis; that of a "
                                  "zero-padded blur (Convolve2D, PSF) is diagonal in neither -- a periodic blur (PeriodicConvolve2D) is")
    if kind in _capi.RADON_KINDS:
        raise NotImplementedError(f"{who} draws x | z exactly where the Hessian of the data term is diagonal in the pixel or the Fourier basis; that of the "
                                  "Radon operator is diagonal in neither (Fourier-domain terms: FourierSampling, PeriodicConvolve2D)")
    if kind == _capi.DATA_SENSE:
        raise NotImplementedError(f"{who} draws x | z exactly where the Hessian of the data term is diagonal in the pixel or the Fourier basis; that of the "
                                  "multi-coil SENSE term (MultiCoilFourierSampling) is diagonal in neither; use MYULA or SK-ROCK")
    if kind in _capi.POISSON_KINDS:
        raise NotImplementedError(f"{who} does not take the Poisson data term: the conditional x | z is not Gaussian")
    if kind in _capi.HUBER_KINDS:
        raise NotImplementedError(f"{who} does not take the Huber data term (HuberLoss): the conditional x | z is not Gaussian")
    if data.get("ncvx_kind", _capi.NCVX_NONE) != _capi.NCVX_NONE:
        raise NotImplementedError(f"{who} does not take the non-convex data terms (L2_ncvx_tv): the conditional x | z is not Gaussian")
    if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
        raise NotImplementedError(f"{who} runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
    if prior.get("tv_warm"):
        raise NotImplementedError(f"{who} has no warm-started TV dual: warm must be off")
    if np.asarray(epsg).size > 1:
        raise NotImplementedError(f"{who} takes a scalar epsg: array-valued epsg belongs to MYULASampler")


def sgs_xstep(proxf, z, rho, noise=None, dims=None):
    """The stateless x-draw of the split Gibbs sampler (``lmc_sgs_xstep``): a draw of ``x | z`` for the images ``z`` (``[n, H, W]`` or ``[H, W]``) with
    the white field ``noise`` of the same shape; ``noise=None`` returns the conditional mean, ``prox_{rho^2 f}(z)``.  numpy in, numpy out; a torch tensor in, a torch tensor on its device out."""
    data = _data_descriptor(proxf)
    _refuse_sgs(data, {}, None, 1.0)
    if not (np.isfinite(float(rho)) and float(rho) > 0):
        raise ValueError(f"rho must be finite and > 0 (got {rho!r})")
    dims = _dims_of(dims, proxf, getattr(proxf, "Op", None))
    prob = _Problem(dims, data, None)
    zt = _dev.to_dev(z, prob.device)
    n = prob.dims[0] * prob.dims[1]
    if zt.numel() % n:
        raise ValueError(f"z of shape {tuple(zt.shape)} is not a batch of {prob.dims} images")
    nt = None if noise is None else _dev.to_dev(noise, prob.device)
    if nt is not None and nt.numel() != zt.numel():
        raise ValueError("noise must have the shape of z")
    out = torch.empty_like(zt)
    _dev.run(zt, "lmc_sgs_xstep", C.byref(prob.c), _dev.ptr(zt), _dev.ptr(nt), _dev.ptr(out), zt.numel() // n, float(rho))
    return _dev.like_input(out, z)


class SplitGibbsSampler:
    """The split Gibbs sampler (Vono, Dobigeon, Chainais 2019) for many chains: owns an ``lmc_sgs`` handle (include/lmc_atomi.h holds the definition).

    Target ``pi_rho(x, z) ~ exp(-f(x) - epsg g(z) - ||x - z||^2 / (2 rho^2))``.  One iteration: an EXACT Gaussian draw of ``x | z`` -- no step size, and
    as well conditioned for a 30 % k-space mask or a PSF with spectral zeros as for the identity -- then ``n_inner`` MYULA steps of size ``tau`` and
    smoothing ``gamma`` on ``z | x`` (:func:`sgs_step_bound` gives the recommended ``tau``).  ``proxf``: :class:`L2` over ``FourierSampling``,
    ``PeriodicConvolve2D``, ``Identity``, ``Diagonal``, ``L2(weights=)`` on the identity, or ``None``; ``proxg``: every prior and ``bounds=`` that
    :class:`MYULASampler` takes without a data term.  The x-marginal is the posterior with ``g`` replaced by a ``rho^2``-smoothed version of it: a bias of
    the model, set by ``rho``, separate from the bias of the MYULA z-step, set by ``tau`` and ``gamma``.  The kept iterate (moments, chain groups) is ``x``.
    Plane ``p`` (0: the noise of the x-draw, 1: of the z-step) draws the Philox field of the seed ``(seed + (p << 32)) mod 2^64``; any sharding of the
    chains by ``chain_offset`` reproduces the same trajectories.  What the library has no path for raises ``NotImplementedError`` before a handle
    exists, bad values ``ValueError``."""

    def __init__(self, proxf, proxg, dims, n_chains, rho, tau, gamma, n_inner=1, epsg=1.0, seed=0, burn_in=0, thin=1, chain_groups=None, chain_offset=0,
                 noise="philox", moments=True, device=None, variant=None):
        data, prior = _data_descriptor(proxf), _prior_descriptor(proxg)
        _refuse_sgs(data, prior, proxg, epsg)
        for name, v in (("rho", rho), ("tau", tau), ("gamma", gamma)):
            if not (np.isfinite(float(v)) and float(v) > 0):
                raise ValueError(f"{name} must be finite and > 0 (got {v!r})")
        if not 1 <= int(n_inner) <= _capi.MAX_SGS_INNER:
            raise ValueError(f"n_inner must be in 1 .. {_capi.MAX_SGS_INNER} (got {n_inner!r})")
        if not float(epsg) >= 0:
            raise ValueError(f"epsg must be >= 0 (got {epsg!r})")
        if noise not in ("philox", "injected", "none"):
            raise ValueError("noise must be 'philox', 'injected' or 'none'")
        if int(n_chains) < 1:
            raise ValueError("n_chains must be >= 1")
        if moments and (int(thin) < 1 or int(burn_in) < 0):
            raise ValueError("thin must be >= 1 and burn_in >= 0")
        self.dims = (int(dims[0]), int(dims[1]))
        if data.get("data_kind") == _capi.DATA_SPECTRAL:
            _capi.check_fft_dims(self.dims)
        groups = _check_chain_groups(chain_groups, moments)
        self.n_chains, self.n_inner = int(n_chains), int(n_inner)
        self.rho, self.tau, self.gamma = float(rho), float(tau), float(gamma)
        self.device = _dev.device(device)
        self.proxf, self.proxg = proxf, proxg
        self._problem = _Problem(self.dims, data, prior, self.device, options={"step_variant": variant or 0})
        cfg = _capi.lmc_sgs_config()
        cfg.struct_size = C.sizeof(_capi.lmc_sgs_config)
        cfg.problem = self._problem.c
        cfg.n_chains = self.n_chains
        cfg.chain_offset = int(chain_offset)
        cfg.rho, cfg.tau, cfg.gamma, cfg.epsg = self.rho, self.tau, self.gamma, float(epsg)
        cfg.n_inner = self.n_inner
        cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.noise_mode = {"philox": _capi.NOISE_PHILOX, "injected": _capi.NOISE_INJECTED, "none": _capi.NOISE_NONE}[noise]
        cfg.moments = 1 if moments else 0
        cfg.burn_in, cfg.thin = int(burn_in), int(thin)
        self.noise_mode, self.moments_on, self.chain_groups = noise, bool(moments), None
        self._h = C.c_void_p()
        torch.cuda.current_stream(self.device).synchronize()      # the problem's arrays are on the device before the handle reads them
        with torch.cuda.device(self.device):
            rc = _dev.lib().lmc_sgs_create(C.byref(cfg), C.byref(self._h))
            if rc == -2:
                raise NotImplementedError(_dev.lib().lmc_last_error().decode())
            if rc == -1:
                raise ValueError(_dev.lib().lmc_last_error().decode())
            _capi.check(rc)
            if groups is not None:
                _capi.check(_dev.lib().lmc_sgs_set_chain_groups(self._h, groups))
                self.chain_groups = groups

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _dev.lib().lmc_sgs_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def shape(self):
        return (self.n_chains,) + self.dims

    def planes(self):
        """Both planes at once, ``[2, n_chains, H, W]`` fp32 on the device: x then z (``state`` and ``aux`` each make this copy and return one of them)."""
        return self._planes()

    def _planes(self):
        out = torch.empty((2,) + self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_sgs_get_state(self._h, _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    @property
    def state(self):
        """x, ``[n_chains, H, W]`` fp32 on the device: the variable whose marginal approximates the posterior."""
        return self._planes()[0]

    @property
    def aux(self):
        """z, ``[n_chains, H, W]`` fp32 on the device: the auxiliary variable that carries the prior."""
        return self._planes()[1]

    def set_state(self, x, z=None):
        """``x`` (and ``z``; default ``z = x``): one image ``[H, W]`` broadcast to every chain, or ``[n_chains, H, W]``."""
        n = self.dims[0] * self.dims[1]
        planes = []
        for a in (x, x if z is None else z):
            t = _dev.to_dev(a, self.device)
            if t.numel() == n:
                t = t.reshape(1, *self.dims).expand(self.shape)
            if t.numel() != self.n_chains * n:
                raise ValueError(f"state of shape {tuple(t.shape)} does not match {self.shape}")
            planes.append(t.reshape(self.shape))
        both = torch.stack(planes).contiguous()
        _capi.check(_dev.lib().lmc_sgs_set_state(self._h, _dev.ptr(both), _dev.stream_ptr(self.device)))
        torch.cuda.current_stream(self.device).synchronize()  # `both` is a temporary

    @property
    def iteration(self):
        return int(_dev.lib().lmc_sgs_iteration(self._h))

    @iteration.setter
    def iteration(self, it):
        _capi.check(_dev.lib().lmc_sgs_set_iteration(self._h, int(it)))

    def step(self, n=1, noise=None):
        """``n`` iterations on every chain.  ``noise`` (only with noise='injected'): ``[n, 1 + n_inner, n_chains, H, W]``, the field of the x-draw first."""
        nt = None
        if noise is not None:
            nt = _dev.to_dev(noise, self.device)
            if nt.numel() != int(n) * (1 + self.n_inner) * int(np.prod(self.shape)):
                raise ValueError("noise must have shape [n, 1 + n_inner, n_chains, H, W]")
        _capi.check(_dev.lib().lmc_sgs_step(self._h, int(n), _dev.ptr(nt), _dev.stream_ptr(self.device)))
        if nt is not None:
            torch.cuda.current_stream(self.device).synchronize()

    @property
    def kernel_name(self):
        return _dev.lib().lmc_sgs_kernel_name(self._h).decode()

    def energies(self):
        """Per-chain ``f(x_c)``, ``g(z_c)`` and the coupling ``||x_c - z_c||^2 / (2 rho^2)`` (float64 tensors in HBM); ``g = 0`` for a prior without a
        value (closed-form proxes, TGV), as elsewhere."""
        f, g, k = (torch.empty(self.n_chains, dtype=torch.float64, device=self.device) for _ in range(3))
        _capi.check(_dev.lib().lmc_sgs_energies(self._h, _dev.ptr(f), _dev.ptr(g), _dev.ptr(k), _dev.stream_ptr(self.device)))
        return f, g, k

    def noise(self, it, plane):
        """The Philox field ``[n_chains, H, W]`` of iteration ``it``: ``plane`` 0 is the noise of the x-draw, ``1 + j`` that of inner z-step ``j``."""
        out = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        _capi.check(_dev.lib().lmc_sgs_noise(self._h, int(it), int(plane), _dev.ptr(out), _dev.stream_ptr(self.device)))
        return out

    def moments(self):
        """(sum [H, W] f64, sumsq [H, W] f64, count) of x over chains and kept iterations."""
        a = torch.empty(self.dims, dtype=torch.float64, device=self.device)
        b = torch.empty_like(a)
        cnt = C.c_uint64()
        _capi.check(_dev.lib().lmc_sgs_get_moments(self._h, _dev.ptr(a), _dev.ptr(b), C.byref(cnt), _dev.stream_ptr(self.device)))
        return a, b, int(cnt.value)

    def reset_moments(self):
        _capi.check(_dev.lib().lmc_sgs_reset_moments(self._h, _dev.stream_ptr(self.device)))

    def group_moments(self):
        """(S1, S2 ``[chain_groups, H, W]`` f64, counts ``[chain_groups]`` int64 CPU tensor) of x, as :meth:`MYULASampler.group_moments`."""
        if self.chain_groups is None:
            raise ValueError("the sampler keeps no chain-group moments (chain_groups=)")
        S1 = torch.empty((self.chain_groups,) + self.dims, dtype=torch.float64, device=self.device)
        S2 = torch.empty_like(S1)
        cnt = (C.c_uint64 * self.chain_groups)()
        _capi.check(_dev.lib().lmc_sgs_get_group_moments(self._h, _dev.ptr(S1), _dev.ptr(S2), cnt, _dev.stream_ptr(self.device)))
        return S1, S2, torch.tensor([int(v) for v in cnt], dtype=torch.int64)


class SplitGibbsResult:
    """Return value of :func:`SplitGibbs`: ``mean`` / ``var`` of x over the kept samples ``[H, W]``, ``state`` (x) and ``aux`` (z) ``[n_chains, H, W]``,
    the per-chain ``energy_f``, ``energy_g``, ``energy_coupling``; with ``chain_groups`` the maps ``mcse_mean`` and ``ess`` (else ``None``)."""

    def __init__(self, mean, var, count, state, aux, energy_f, energy_g, energy_coupling, elapsed, mcse_mean=None, ess=None):
        self.mean, self.var, self.count, self.state, self.aux = mean, var, count, state, aux
        self.energy_f, self.energy_g, self.energy_coupling, self.elapsed = energy_f, energy_g, energy_coupling, elapsed
        self.mcse_mean, self.ess = mcse_mean, ess


def SplitGibbs(proxf, proxg, x0, rho, tau, gamma, niter, n_chains=1, n_inner=1, epsg=1.0, seed=0, burn_in=0, thin=1, chain_groups=None, chain_offset=0,
               dims=None, device=None):
    """``niter`` iterations of :class:`SplitGibbsSampler` from ``x = z = x0`` (``[H, W]`` or ``[n_chains, H, W]``); returns a :class:`SplitGibbsResult`."""
    dims = _dims_of(dims, proxg, proxf, getattr(proxf, "Op", None))
    if chain_groups is not None:
        _check_chain_groups(chain_groups, True, n_chains)
    smp = SplitGibbsSampler(proxf, proxg, dims, n_chains, rho, tau, gamma, n_inner=n_inner, epsg=epsg, seed=seed, burn_in=burn_in, thin=thin,
                            chain_groups=chain_groups, chain_offset=chain_offset, device=device)
    with smp:
        smp.set_state(x0)
        tstart = time.time()
        smp.step(niter)
        s1, s2, cnt = smp.moments()
        f, g, k = smp.energies()
        planes = smp._planes()
        groups = _group_summaries(smp)
        torch.cuda.current_stream(smp.device).synchronize()
        mean, var = mean_var_from_moments(s1, s2, max(cnt, 1))
        return SplitGibbsResult(mean, var, cnt, planes[0], planes[1], f, g, k, time.time() - tstart,
                                mcse_mean=None if groups is None else groups[0], ess=None if groups is None else groups[2])


class MYMALASampler(MYULASampler):
    """Metropolis-adjusted MYULA (MYMALA) for many chains at image scale: the accept / reject of the reference's toy
    ``ProximalLangevinMonteCarlo.mymala`` (prox_lmc.py:134-158) generalised to ``[C, H, W]`` states, everything on the device.
    Same constructor as :class:`MYULASampler`; a rejected chain keeps its state (and is counted again by the moments)."""

    _create_fn = "lmc_mymala_create"

    _box_refusal = ("MYMALA", "its target would be +infinity outside the box, where MYULA's proposals land; use MYULA")
    _term_refusal = {"poisson": ("MYMALA", "its Metropolis ratio needs the energy by-products of the step, which the Poisson kernels do not form; use MYULA or SK-ROCK")}
    _psf_refusal = ("MYMALA", "its Metropolis ratio is pinned for the fused step, which the three-launch PSF step is not; use MYULA or SK-ROCK")
    _spectral_refusal = ("MYMALA", "its Metropolis ratio is pinned for the fused step, which the three-launch spectral step is not; use MYULA or SK-ROCK")
    _radon_refusal = ("MYMALA", "its Metropolis ratio is pinned for the fused step, which the three-launch Radon step is not; use MYULA or SK-ROCK")
    _sense_refusal = ("MYMALA", "its Metropolis ratio is pinned for the fused step, which the coil-by-coil SENSE step is not; use MYULA or SK-ROCK")
    _eprox_refusal = ("MYMALA", "the prior has a prox and no value g(x), so the Metropolis target exp(-f - epsg g) is undefined; use MYULA")

    def acceptance(self):
        """(accepted proposals per chain [C] int64 tensor, log acceptance ratio of the last iteration [C] float64 tensor)."""
        acc = torch.empty(self.n_chains, dtype=torch.int64, device=self.device)
        la = torch.empty(self.n_chains, dtype=torch.float64, device=self.device)
        _capi.check(_dev.lib().lmc_sampler_get_acceptance(self._h, _dev.ptr(acc), _dev.ptr(la), _dev.stream_ptr(self.device)))
        return acc, la

    def acceptance_rate(self):
        acc, _ = self.acceptance()
        return acc.double() / max(self.iteration, 1)


def MoreauYosidaMetropolisAdjustedLangevin(proxf, proxg, x0, tau=None, gamma=.1, epsg=1., niter=10, seed=0, callback=None, *,
                                           n_chains=1, dims=None, chain_offset=0, burn_in=0, thin=1, device=None, moment_scales=None,
                                           hist_bins=None, hist_range=None, quantiles=(0.05, 0.5, 0.95), chain_groups=None, cov_probes=None, cov_center=None):
    """MYMALA at image scale for ``n_chains`` chains (the accept / reject of prox_lmc.py:134-158 around the MYULA move of
    algs.py:569): returns a :class:`MYULAResult` with two extra attributes, ``accepted`` (per-chain counts) and
    ``acceptance_rate``.  ``callback(state)`` after every iteration if given.  ``moment_scales``, ``hist_bins`` / ``hist_range`` /
    ``quantiles``, ``chain_groups``, ``cov_probes`` / ``cov_center``: as in :func:`MoreauYosidaUnadjustedLangevin`."""
    dims = _dims_of(dims, proxf, proxg)
    acc = _accumulator_keywords(locals(), True, n_chains, dims)
    with MYMALASampler(proxf, proxg, dims, n_chains=int(n_chains), tau=tau, gamma=gamma, epsg=epsg, seed=seed,
                       chain_offset=chain_offset, moments=True, burn_in=burn_in, thin=thin, device=device, **acc) as smp:
        tstart = _run(smp, x0, niter, callback)
        accepted, _ = smp.acceptance()
        res = _result(smp, quantiles, tstart)
        res.accepted = accepted
        res.acceptance_rate = accepted.double() / max(niter, 1)
        return res


def skrock_coefficients(n_stages, eta=0.05):
    """``(mu, nu, kappa)`` of SK-ROCK with ``n_stages`` stages and damping ``eta``: float64 arrays, entry ``j - 1`` = stage ``j``, as the library
    forms them (``lmc_skrock_coefficients``; the definition is in include/lmc_atomi.h).  Needs no GPU.  ``n_stages`` outside 2 .. 64 or an ``eta``
    that is not finite and positive raises ``ValueError``."""
    mu, nu, kappa, _ = _skrock_coefficients(n_stages, eta)
    return mu, nu, kappa


def _skrock_coefficients(n_stages, eta):
    s = int(n_stages)
    n = min(max(s, 1), _capi.MAX_SKROCK_STAGES)
    mu, nu, kappa = (np.zeros(n, dtype=np.float64) for _ in range(3))
    ls = C.c_double()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _dev.lib().lmc_skrock_coefficients(s, float(eta), dp(mu), dp(nu), dp(kappa), C.byref(ls))
    if rc == -1:       # LMC_E_INVALID
        raise ValueError(_dev.lib().lmc_last_error().decode("utf-8", "replace"))
    _capi.check(rc)
    return mu, nu, kappa, float(ls.value)


def skrock_step_bound(L, n_stages, eta=0.05):
    """Largest stable step of SK-ROCK for a drift with Lipschitz constant ``L`` (``L_f + 1 / gamma`` for the MYULA drift):
    ``l_s / L`` with ``l_s = (s - 1/2)^2 (2 - 4 eta / 3) - 3/2``, where MYULA stops near ``1 / L``."""
    return _skrock_coefficients(n_stages, eta)[3] / float(L)


class SKROCKSampler(MYULASampler):
    """SK-ROCK for many chains at image scale (Pereyra, Vargas Mieles, Zygalakis 2020): ``n_stages`` evaluations of the MYULA drift per iteration,
    each one launch of the fused step kernel with Chebyshev coefficients, stable up to ``tau = skrock_step_bound(L, n_stages, eta)`` --
    integrated time per gradient evaluation grows like ``n_stages``.  The other arguments are :class:`MYULASampler`'s; one noise field per
    iteration (``step(n, noise=[n, C, H, W])`` with ``noise='injected'``), ``iteration`` counts iterations, not stages.  ``TV(rtol > 0)``,
    a warm-started TV dual and array-valued ``epsg`` run outside the fused launch and raise ``NotImplementedError``."""

    def __init__(self, proxf, proxg, dims, n_stages=10, eta=0.05, **kw):
        _check_accumulators(kw, kw.get("moments", False), dims)      # before anything touches the proxes
        prior = _prior_descriptor(proxg)
        _refuse_box(prior, "SK-ROCK", "its stability bound is derived for the unconstrained Moreau-Yosida envelope; use MYULA")
        if float(prior.get("tv_rtol", 0.0) or 0.0) > 0.0:
            raise NotImplementedError("SK-ROCK runs the fixed-count TV prox: TV(rtol > 0) is not built for it")
        if prior.get("tv_warm") or kw.get("tv_warm"):
            raise NotImplementedError("SK-ROCK evaluates the drift at n_stages points per iteration: a warm-started TV dual (warm=True) is not built for it")
        if np.asarray(kw.get("epsg", 1.0)).size > 1:
            raise NotImplementedError("SK-ROCK takes a scalar epsg (array-valued epsg is MYULA's)")
        _skrock_coefficients(n_stages, eta)          # ValueError for a stage count or damping the library refuses
        self.n_stages, self.eta = int(n_stages), float(eta)
        super().__init__(proxf, proxg, dims, **kw)

    def _create(self, cfg):
        return _dev.lib().lmc_skrock_create(C.byref(cfg), self.n_stages, self.eta, C.byref(self._h))


def StabilisedLangevin(proxf, proxg, x0, tau, gamma=.1, epsg=1., niter=10, n_stages=10, eta=0.05, seed=0, callback=None, *,
                       n_chains=1, dims=None, chain_offset=0, burn_in=0, thin=1, device=None, moment_scales=None,
                       hist_bins=None, hist_range=None, quantiles=(0.05, 0.5, 0.95), chain_groups=None, cov_probes=None, cov_center=None):
    """SK-ROCK at image scale for ``n_chains`` chains (:class:`SKROCKSampler`): ``niter`` iterations of ``n_stages`` drift evaluations each at
    step ``tau`` (up to :func:`skrock_step_bound`).  Returns a :class:`MYULAResult` with two extra attributes, ``n_stages`` and
    ``gradient_evaluations = niter * n_stages``.  ``callback(state)`` after every iteration if given.  ``moment_scales``, ``hist_bins`` /
    ``hist_range`` / ``quantiles``, ``chain_groups``, ``cov_probes`` / ``cov_center``: as in :func:`MoreauYosidaUnadjustedLangevin`."""
    dims = _dims_of(dims, proxf, proxg)
    acc = _accumulator_keywords(locals(), True, n_chains, dims)
    with SKROCKSampler(proxf, proxg, dims, n_stages=n_stages, eta=eta, n_chains=int(n_chains), tau=tau, gamma=gamma, epsg=epsg, seed=seed,
                       chain_offset=chain_offset, moments=True, burn_in=burn_in, thin=thin, device=device, **acc) as smp:
        res = _result(smp, quantiles, _run(smp, x0, niter, callback))
        res.n_stages = smp.n_stages
        res.gradient_evaluations = int(niter) * smp.n_stages
        return res


def EstimatePriorWeight(proxf, proxg, x0, tau, gamma, n_updates, theta_bounds, theta0=None, warmup=0, iters_per_update=1, step_scale=10.,
                        step_exponent=0.8, average_from=None, dim_eff=None, epsg=1., seed=0, *, n_chains=1, sampler="myula", n_stages=10, eta=0.05,
                        dims=None, chain_offset=0, device=None):
    """Empirical-Bayes weight of ``proxg`` in one call: a :class:`MYULASampler` (``sampler='myula'``) or :class:`SKROCKSampler`
    (``'skrock'``, ``n_stages`` / ``eta``) of ``n_chains`` chains started at ``x0``, then :meth:`MYULASampler.estimate_prior_weight`.
    Returns its :class:`SAPGResult` with the final ``state`` ``[n_chains, H, W]``.  The gradient estimate is the mean of the prior value over
    the chains, so many chains help directly.  Argument errors (bounds, ``theta0`` outside them, exponent outside (0.5, 1]) raise ``ValueError``
    and unsupported combinations ``NotImplementedError``, both before a sampler exists."""
    if sampler not in ("myula", "skrock"):
        raise NotImplementedError(f"sampler {sampler!r}: the weight is estimated with 'myula' or 'skrock' (MYMALA caches its Metropolis energy, "
                                  "ULPDA has no setter)")
    _refuse_vtv(proxg, "EstimatePriorWeight")
    dims = _dims_of(dims, proxf, proxg)
    prior = _prior_descriptor(proxg)
    _refuse_tgv(prior, "EstimatePriorWeight", "its value g(x), the statistic of the estimator, is a minimisation over the auxiliary field and is not built")
    _refuse_box(prior, "EstimatePriorWeight", "the d / k homogeneity argument of the estimator does not hold on a bounded set")
    if theta0 is None:
        theta0 = _prior_weight(proxg)
    _sapg_config(n_updates, theta_bounds, theta0, warmup, iters_per_update, step_scale, step_exponent, average_from, dim_eff)
    if prior["prior_kind"] in (_capi.PRIOR_NONE, _capi.PRIOR_EPROX):
        raise NotImplementedError(f"{type(proxg).__name__} has no value g(x): its weight cannot be estimated")
    if prior.get("tv_warm"):
        raise NotImplementedError("a warm-started TV dual (warm=True) belongs to the weight it was formed with: the weight cannot move")
    if np.asarray(epsg).size > 1:
        raise NotImplementedError("array-valued epsg carries the weights itself: the scalar weight cannot be estimated")
    kw = dict(n_chains=int(n_chains), tau=tau, gamma=gamma, epsg=epsg, seed=seed, chain_offset=chain_offset, device=device)
    smp = SKROCKSampler(proxf, proxg, dims, n_stages=n_stages, eta=eta, **kw) if sampler == "skrock" else MYULASampler(proxf, proxg, dims, **kw)
    with smp:
        smp.set_state(x0)
        res = smp.estimate_prior_weight(n_updates, theta_bounds, theta0=theta0, warmup=warmup, iters_per_update=iters_per_update,
                                        step_scale=step_scale, step_exponent=step_exponent, average_from=average_from, dim_eff=dim_eff)
        res.state = smp.get_state()
        torch.cuda.current_stream(smp.device).synchronize()
        return res


def set_cg_tolerance(tol=1e-6):
    """Relative residual at which the inner CG solver of the implicit data step stops early (the reference's solver, scipy
    lsqr, stops at btol = 1e-6 by default, algs.py:250); 0 = always run ``niter`` iterations.  Returns the previous value."""
    return float(_dev.lib().lmc_set_cg_tolerance(float(tol)))


def set_step_variant(variant="auto"):
    """Library-wide DEFAULT of the step-kernel variant ('auto' | 'tile' | 'split' | 'point' | 'block' | 'rows' | 'pipe' | 'pipe2'; 'pipe' is the
    pipeline in its one-team layout, 'pipe2' in its two-team layout); returns the previous one.  Process-global, for A/B tests and profiles; a sampler's own ``variant=`` argument takes precedence.  All compute the same update."""
    names = _capi.VARIANTS
    if variant not in names or variant.startswith("("):
        raise ValueError(f"unknown step-kernel variant {variant!r} (the one-group 'stream' kernel of ABI 1 was removed)")
    prev = _dev.lib().lmc_set_step_variant(names.index(variant))
    if prev < 0:
        _capi.check(prev)
    return names[prev]
