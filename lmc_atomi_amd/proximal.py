"""Prox-operator plugin surface (pyproximal ``ProxOperator`` protocol as consumed by
algs.py: ``obj(x)`` :461,578 ; ``obj.prox(x, tau)`` :440,569 ; ``obj.proxdual(x, tau)`` :436,448 ;
``obj.grad(x)`` :569), computed by HIP kernels through the C ABI.

Every class also exposes ``descriptor()``: the plain-data description the fused sampler
kernels are configured from (``lmc_problem`` in include/lmc_atomi.h).  A device-side
function-pointer plugin ABI is deliberately not offered (it would defeat fusion); new proxes
are added as functors compiled into the library.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _capi, _dev
from .operators import (PSF, Convolve2D, Diagonal, FourierSampling, Identity, LinearOperator, MultiCoilFourierSampling, PeriodicConvolve2D, Radon, _minus_k,
                        spectral_tables)


_warned_pass_by_pass = False


def _exit_lands_on_passes(W, tv_rtol, ncvx_rtol, exit_path):
    """Whether a problem with an early exit (``TV(rtol > 0)`` / isotropic ``L2_ncvx_tv(rtol > 0)``) that did not ask for the pass-by-pass path
    gets it all the same: images up to 128 columns wide, which the full-width pipeline (and with it the exit decided on the device) does not cover."""
    return exit_path == 0 and W <= 128 and (tv_rtol > 0.0 or ncvx_rtol > 0.0)


def _warn_pass_by_pass(W):
    """Once per process: the pass-by-pass early exit synchronises the stream after every pass."""
    global _warned_pass_by_pass
    if _warned_pass_by_pass:
        return
    _warned_pass_by_pass = True
    warnings.warn(f"rtol > 0 on an image {W} columns wide: the early exit of the TV prox is decided pass by pass (one launch per pass for the iterate, one "
                  "for its objective, and a host read that synchronises the stream after every pass); it is decided on the device, without "
                  "synchronisation, on images wider than 128 columns.  exit_path='passes' asks for this path explicitly (no warning).",
                  RuntimeWarning, stacklevel=3)


def fgp_betas(niter, momentum="unlocbox"):
    """Momentum table beta_k = (t_{k-1}-1)/t_k of the TV dual iteration.  'unlocbox' is the
    sequence pyproximal.TV inherits from UNLocBoX [upstream]; 'fista' the textbook one."""
    t, out = 1.0, []
    for _ in range(int(niter)):
        if momentum == "unlocbox":
            tn = (1.0 + np.sqrt(4.0 * t * t)) / 2.0
        elif momentum == "fista":
            tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        elif momentum == "none":
            tn = 1.0
        else:
            raise ValueError(f"unknown momentum {momentum!r}")
        out.append((t - 1.0) / tn)
        t = tn
    return np.asarray(out, dtype=np.float32)


def check_bounds(bounds):
    """``bounds=None`` or ``(lo, hi)`` with ``lo < hi``, neither NaN; infinite ends are allowed (``(0, inf)`` is positivity).  Returns None or the pair of
    floats; anything else raises ``ValueError``."""
    if bounds is None:
        return None
    try:
        lo, hi = (float(v) for v in bounds)
    except (TypeError, ValueError):
        raise ValueError(f"bounds must be None or a pair (lo, hi) (got {bounds!r})") from None
    if lo != lo or hi != hi or not lo < hi:
        raise ValueError(f"bounds: need lo < hi, neither NaN (got ({lo}, {hi}))")
    return lo, hi


def _with_box(desc, bounds):
    """The prior descriptor ``desc`` with the box constraint ``bounds`` (None: as it is)."""
    if bounds is not None:
        desc["box"] = bounds
    return desc


def _box_prox(op, x, tau):
    """``clip(prox_{tau g}(x), lo, hi)`` of a separable prior with bounds -- the prox of g + the indicator of the box -- through ``lmc_fused_eval`` (one
    elementwise launch forms it).  Arrays with two or more axes are batches of images on the last two; anything else is one row."""
    shape = tuple(np.shape(x)) if not isinstance(x, torch.Tensor) else tuple(x.shape)
    n = int(np.prod(shape)) if shape else 1
    dims = (int(shape[-2]), int(shape[-1])) if len(shape) >= 2 else (1, n)
    key = (dims, x.device if isinstance(x, torch.Tensor) and x.is_cuda else None)
    cache = op.__dict__.setdefault("_box_problems", {})
    if key not in cache:
        cache[key] = _Problem(dims, prior=op.prior_descriptor(), dev=key[1])
    return cache[key].eval(x, 0.0, 0.0, 1.0, float(tau))


class ProxOperator:
    """Base class; subclassing hook mirrors ``super().__init__(Op, hasgrad)`` (algs.py:132)."""

    def __init__(self, Op=None, hasgrad=False):
        self.Op = Op
        self.hasgrad = hasgrad

    def proxdual(self, x, tau):
        """Moreau identity (prox.py:9-10): prox_{tau f*}(x) = x - tau prox_{f/tau}(x/tau)."""
        return x - tau * self.prox(x / tau, 1.0 / tau)

    def descriptor(self):
        raise NotImplementedError(f"{type(self).__name__} has no device functor")


class _Problem:
    """Assembles an ``lmc_problem`` from a data-term descriptor and a prior descriptor and keeps
    every buffer it points to alive."""

    def __init__(self, dims, data=None, prior=None, dev=None, options=None):
        if (prior or {}).get("prior_kind") == _capi.PRIOR_VTV and not (options or {}).get("multichannel"):
            raise NotImplementedError("VectorialTV acts on multi-channel images: it is built for MultichannelMYULASampler / MoreauYosidaUnadjustedLangevin and "
                                      "for its own prox and value only; MYMALA, SK-ROCK, ULPDA, the estimation of the prior weight and the single-plane "
                                      "MYULASampler are not built for it")
        self.dims = (int(dims[0]), int(dims[1]))
        self.device = _dev.device(dev)
        dev = self.device
        p = _capi.lmc_problem()
        p.struct_size = C.sizeof(_capi.lmc_problem)
        p.H, p.W = self.dims
        self._keep = []
        data = data or {"data_kind": _capi.DATA_NONE}
        prior = prior or {"prior_kind": _capi.PRIOR_NONE}
        p.data_kind = data["data_kind"]
        p.sigma_f = float(data.get("sigma_f", 0.0))
        if data.get("y") is not None:
            # (a Poisson term: [2][H][W], the counts then the background; a weighted Gaussian term: the observation then the weights; a Huber term: the observation then the thresholds)
            if p.data_kind == _capi.DATA_SPECTRAL:      # the spectral term: the [11][H][W / 2 + 1] planes of lmc_spectral_tables
                y = _dev.to_dev(data["y"], dev).reshape(_capi.SPECTRAL_PLANES, self.dims[0], self.dims[1] // 2 + 1)
            elif p.data_kind == _capi.DATA_SENSE:       # the SENSE term: the mask, the maps and the data of every coil
                y = _dev.to_dev(data["y"], dev).reshape((1 + 4 * int(data["n_coils"]),) + self.dims)
            elif p.data_kind in _capi.RADON_KINDS:      # the Radon operator: sinogram-shaped planes, one (Gaussian) or two (the other terms)
                y = _dev.to_dev(data["y"], dev).reshape(((2,) if p.data_kind != _capi.DATA_RADON else ()) + (len(data["angles"]), int(data["n_det"])))
            else:
                y = _dev.to_dev(data["y"], dev).reshape(((2,) if p.data_kind in _capi.TWO_PLANE_KINDS else ()) + self.dims)
            self._keep.append(y)
            p.y_dev = y.data_ptr()
        if data.get("mask") is not None:
            m = _dev.to_dev(data["mask"], dev).reshape(self.dims)
            self._keep.append(m)
            p.mask_dev = m.data_ptr()
        if p.data_kind in (_capi.DATA_BLUR, _capi.DATA_POISSON_BLUR, _capi.DATA_WL2_BLUR, _capi.DATA_HUBER_BLUR):
            h = np.ascontiguousarray(data["h"], dtype=np.float32)
            self._keep.append(h)
            p.kh, p.kw = h.shape
            p.oy, p.ox = data["offset"]
            p.h_host = _dev.fptr(h)
        if p.data_kind in _capi.PSF_KINDS:      # the large PSF: its geometry in fields of its own (kh = kw = oy = ox = 0), the taps at h_host
            h = np.ascontiguousarray(data["h"], dtype=np.float32)
            self._keep.append(h)
            p.psf_kh, p.psf_kw = h.shape
            p.psf_oy, p.psf_ox = data["offset"]
            p.h_host = _dev.fptr(h)
            p.psf_separable = int(data.get("psf_separable", 0))
        if p.data_kind in _capi.RADON_KINDS:      # the Radon operator rides in fields it does not otherwise read: kh = n_angles, kw = n_det, h_host = the angles
            ang = np.ascontiguousarray(data["angles"], dtype=np.float32)
            self._keep.append(ang)
            p.kh, p.kw = ang.size, int(data["n_det"])
            p.h_host = _dev.fptr(ang)
        if p.data_kind == _capi.DATA_SENSE:       # likewise: kh = n_coils
            p.kh = int(data["n_coils"])
        p.prior_kind = prior["prior_kind"]
        p.prior_sigma = float(prior.get("prior_sigma", 0.0))
        # (ULPDA's anisotropic descriptor carries no prox: tv_niter stays 0)
        if p.prior_kind in (_capi.PRIOR_TV_ISO, _capi.PRIOR_VTV) or (p.prior_kind == _capi.PRIOR_TV_ANISO and prior.get("tv_niter") is not None):
            p.tv_niter = int(prior["tv_niter"])
            p.tv_step = float(prior.get("tv_step", 0.125))
            b = np.ascontiguousarray(prior["tv_betas"], dtype=np.float32)
            if b.size != p.tv_niter:
                raise ValueError("tv_betas must have tv_niter entries")
            self._keep.append(b)
            p.tv_betas_host = _dev.fptr(b)
        p.ncvx_kind = int(data.get("ncvx_kind", _capi.NCVX_NONE))
        p.ncvx_lambda = float(data.get("ncvx_lambda", 0.0))
        p.ncvx_gamma = float(data.get("ncvx_gamma", 1.0))
        p.ncvx_niter = int(data.get("ncvx_niter", 0))
        # ABI 2: which truncated iterate the TV prox returns, warm-started dual, per-problem kernel variant / solver tolerance
        opt = dict(options or {})
        p.tv_lagged_output = 1 if (prior.get("tv_lagged_output") or data.get("tv_lagged_output") or opt.get("tv_lagged_output")) else 0
        p.tv_rtol = float(prior.get("tv_rtol", 0.0) or 0.0)      # > 0: the exact early-exit path of the TV prior's prox (slow; 0 = fixed count)
        p.tv_warm = 1 if (prior.get("tv_warm") or opt.get("tv_warm")) else 0
        v = opt.get("step_variant", 0) or 0
        p.step_variant = _capi.VARIANTS.index(v) if isinstance(v, str) else int(v)
        p.implicit_tol = float(opt.get("implicit_tol", data.get("implicit_tol", 0.0)) or 0.0)
        # ABI 3: early exit of the ME-TV inner prox, which of the two exit paths, launch policy (0 = the library decides)
        p.ncvx_rtol = float(data.get("ncvx_rtol", 0.0) or 0.0)
        p.tv_exit_path = int(prior.get("tv_exit_path", 0) or opt.get("tv_exit_path", 0) or 0)
        if _exit_lands_on_passes(p.W, p.tv_rtol if p.prior_kind == _capi.PRIOR_TV_ISO else 0.0,
                                 p.ncvx_rtol if p.ncvx_kind == _capi.NCVX_ME_TV else 0.0, p.tv_exit_path):
            _warn_pass_by_pass(p.W)
        p.iterations_per_launch = int(opt.get("iterations_per_launch", 0) or 0)
        p.moments_overlap = int(opt.get("moments_overlap", 0) or 0)
        p.moments_bg_workgroups = int(opt.get("moments_bg_workgroups", 0) or 0)
        p.graph_replay = 1 if opt.get("graph_replay") else 0
        if p.prior_kind == _capi.PRIOR_WAVELET_L1:      # its two parameters ride in fields the kind does not otherwise read
            p.tv_niter, p.eprox_kind = int(prior["wavelet_levels"]), int(prior["wavelet_p"])
        if p.prior_kind == _capi.PRIOR_TGV:      # likewise: the iterations, alpha0 and the step of its prox
            p.tv_niter, p.eprox_p0, p.tv_step = int(prior["tgv_niter"]), float(prior["tgv_alpha0"]), float(prior.get("tgv_step", 0.0))
        if p.prior_kind == _capi.PRIOR_EPROX:
            p.eprox_kind = int(prior["eprox_kind"])
            p.eprox_p0, p.eprox_p1 = float(prior["eprox_p0"]), float(prior["eprox_p1"])
            p.eprox_scale_mask = int(prior.get("eprox_scale_mask", 0))
        if opt.get("prox_scale") is not None:     # array-valued epsg (MYULA): device array + (chain, pixel) strides
            sc, cs, ps = opt["prox_scale"]
            self._keep.append(sc)
            p.prox_scale, p.prox_scale_chain_stride, p.prox_scale_pixel_stride = _dev.ptr(sc), int(cs), int(ps)
        if prior.get("box") is not None:          # x in [lo, hi]: the prox is that of g + the indicator of the box
            p.box_enable = 1
            p.box_lo, p.box_hi = check_bounds(prior["box"])
        self.c = p

    def eval(self, x, a, t, b, pt):
        """out = a*x - t*grad f(x) + b*prox_{pt*g}(x) for image-shaped / flat batches."""
        n = self.dims[0] * self.dims[1]
        xt = _dev.to_dev(x, self.device)
        if xt.numel() % n:
            raise ValueError(f"operand of shape {tuple(xt.shape)} is not a batch of {self.dims} images")
        out = torch.empty_like(xt)
        with torch.cuda.device(self.device):       # the problem's buffers (y, mask) live there
            _dev.run(xt, "lmc_fused_eval", C.byref(self.c), _dev.ptr(xt), _dev.ptr(out), xt.numel() // n,
                                                  a, t, b, pt)
        return _dev.like_input(out, x)

    def energies(self, x):
        n = self.dims[0] * self.dims[1]
        xt = _dev.to_dev(x, self.device)
        n_img = xt.numel() // n
        f = torch.empty(n_img, dtype=torch.float64, device=xt.device)
        g = torch.empty(n_img, dtype=torch.float64, device=xt.device)
        with torch.cuda.device(self.device):
            _dev.run(xt, "lmc_energies", C.byref(self.c), _dev.ptr(xt), n_img, _dev.ptr(f), _dev.ptr(g))
        return f, g


class L2(ProxOperator):
    """``f(x) = sigma/2 ||Op x - b||^2`` -- drop-in for ``pyproximal.L2(Op=H, b=y, sigma=1/sigma**2,
    niter=50, warm=True)`` (prox_lmc_deconv.py:101-103) and for the prior ``pyproximal.L2(sigma=lam)``.

    ``Op`` may be a :class:`Convolve2D`, :class:`Diagonal`, :class:`Identity` or ``None``.
    ``grad`` runs the fused blur-residual-adjoint kernel; value via the energy kernel.
    The implicit step ``prox`` with an operator (row a8 of SURVEY section 8, used by ULPDA only) is
    provided by :mod:`lmc_atomi_amd.algs` for ULPDA; for ``Op is None`` it is closed form.

    ``weights`` (build extension; ``LMC_DATA_WL2_*`` in include/lmc_atomi.h is its definition): an ``[H, W]`` or flat array ``w >= 0`` of the image's
    size gives ``f(x) = sigma/2 sum_p w_p ((Op x)_p - b_p)^2`` with ``grad f = sigma Op^T(w * (Op x - b))`` -- a pixel with ``w_p = 0`` is unobserved
    (dead or saturated pixels under a blur, a masked-out border), ``w_p = 1 / sigma_p^2`` is a noise map.  ``Op``: :class:`Convolve2D`,
    :class:`Identity` or ``None``; a binary mask on a blur is ``weights = mask`` (``Diagonal`` with weights is refused).  As ``proxf`` of MYULA, MYMALA,
    SK-ROCK and :func:`EstimatePriorWeight`; ``prox``, ULPDA, ``TV(rtol > 0)``, ``TV(warm=True)``, the block-Haar :class:`WaveletL1` and a forced kernel variant other
    than 'auto' / 'tile' / 'pipe' raise ``NotImplementedError``.  ``weights=None`` is the unweighted term, unchanged.
    """

    def __init__(self, Op=None, b=None, sigma=1.0, niter=10, warm=True, dims=None, bounds=None, weights=None):
        super().__init__(Op, True)
        self.bounds = check_bounds(bounds)        # as the prior only: sigma/2 ||x||^2 + the indicator of [lo, hi]
        if self.bounds is not None and (Op is not None or b is not None):
            raise NotImplementedError("bounds belong to the prior: only L2(sigma=...) without Op / b takes them")
        self.b = b
        self.sigma = float(sigma)
        self.niter = niter
        self.warm = warm
        self.dims = dims if dims is not None else getattr(Op, "dims", None)
        self._prob = None
        self._x0 = None          # warm-start vector of the implicit step (stateful, as the reference's L2)
        self.weights = None
        self._spectral = None
        if isinstance(Op, (FourierSampling, PeriodicConvolve2D)):
            self._set_spectral(weights)
        elif isinstance(Op, Radon):
            self._set_radon(weights)
        elif isinstance(Op, MultiCoilFourierSampling):
            self._set_sense(weights)
        elif weights is not None:
            self._set_weights(weights)

    def _set_radon(self, weights):
        """The Gaussian terms on the Radon operator (``LMC_DATA_RADON`` / ``LMC_DATA_WL2_RADON``): ``b`` and ``weights`` live on the sinogram."""
        if self.b is None:
            raise ValueError("L2 with Radon needs b: the sinogram")
        self.dims = self.Op.dims
        y = _sino_plane(self.Op, self.b, "L2", "b")
        if not np.all(np.isfinite(y)):
            raise ValueError("L2 with Radon: b must be finite (mark a bad bin with weight 0, not with NaN)")
        self._sino = np.ascontiguousarray(y, dtype=np.float32)
        if weights is not None:
            w = _sino_plane(self.Op, weights, "L2", "weights")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("L2: the weights must be finite and >= 0 (0 marks an unobserved bin)")
            self.weights = w
            self._yw = np.ascontiguousarray(np.stack([y, w]), dtype=np.float32)      # [2][n_angles][n_det]: what y_dev points to
            self._yw_dev = {}

    def _set_sense(self, weights):
        """The multi-coil SENSE data term (``LMC_DATA_SENSE``): the mask, the maps and the complex data of every coil as the planes ``y_dev`` points to."""
        if weights is not None:
            raise NotImplementedError("L2(weights=...) with MultiCoilFourierSampling: a weight per frequency is the operator's mask (mask = sqrt(w), b * sqrt(w))")
        if self.b is None:
            raise ValueError("L2 with MultiCoilFourierSampling needs b: the k-space measurements [n_coils, H, W]")
        self.dims = self.Op.dims
        self._sense = self.Op.descriptor(self.b)
        self._sense_dev = {}

    def _sense_buffer(self):
        """The planes on the current device, uploaded once (per device) and kept alive by this object."""
        key = _dev.device(None)
        if key not in self._sense_dev:
            self._sense_dev[key] = _dev.to_dev(self._sense, key)
        return self._sense_dev[key]

    def _set_spectral(self, weights):
        """The Fourier-domain data term (``LMC_DATA_SPECTRAL``): G and b of the operator, ``weights`` per frequency as G sqrt(w) and b sqrt(w), folded once on
        the host into the planes ``y_dev`` points to."""
        if self.b is None:
            raise ValueError(f"L2 with {type(self.Op).__name__} needs b: the measurements")
        self.dims = self.Op.dims
        G, b = self.Op.gain(), self.Op.data(self.b)
        if weights is not None:
            w = _host(weights).astype(np.float64)
            if w.size != G.size or w.ndim not in (1, 2) or (w.ndim == 2 and w.shape != self.dims):
                raise ValueError(f"L2: weights of shape {w.shape} for the full plane {self.dims} (one weight per frequency)")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("L2: the weights must be finite and >= 0")
            rw = np.sqrt(w.reshape(self.dims))
            G, b = G * rw, b * rw
        self._spectral = {"G": G, "b": b, "tab": spectral_tables(G, b), "dev": {}}
        self._amax = float(np.max(0.5 * (np.abs(G) ** 2 + np.abs(_minus_k(G)) ** 2)))

    def _spectral_buffer(self):
        """The planes on the current device, uploaded once (per device) and kept alive by this object."""
        key = _dev.device(None)
        if key not in self._spectral["dev"]:
            self._spectral["dev"][key] = _dev.to_dev(self._spectral["tab"], key)
        return self._spectral["dev"][key]

    def _set_weights(self, weights):
        """Validates the per-pixel weights and builds the [2][H][W] host array (observation, weights) that ``y_dev`` points to."""
        if isinstance(self.Op, Diagonal):
            raise NotImplementedError("L2(weights=...) with Op = Diagonal: there is no weighted mask kind -- a binary mask m on a blur is weights = m")
        if self.b is None:
            raise NotImplementedError("L2(weights=...) without b: the weights belong to the data term; as a prior they have no meaning")
        if self.Op is not None and not isinstance(self.Op, (Convolve2D, PSF, Identity)):
            raise NotImplementedError(f"no device functor for L2(weights=...) with Op of type {type(self.Op).__name__} (Convolve2D, PSF or Identity)")
        w = _host(weights).astype(np.float64)
        y = _host(self.b).astype(np.float64)
        if self.dims is None:      # the image shape: `dims`, else the operator's, else that of an [H, W] array of weights or observations
            for cand in (w.shape if w.ndim == 2 else None, y.shape if y.ndim == 2 else None):
                if cand is not None:
                    self.dims = cand
                    break
            else:
                raise ValueError("L2(weights=...): image shape unknown (Op carries none, b and weights are flat): pass dims=(ny, nx)")
        self.dims = (int(self.dims[0]), int(self.dims[1]))
        n = self.dims[0] * self.dims[1]
        if w.size != n or w.ndim not in (1, 2) or (w.ndim == 2 and w.shape != self.dims):
            raise ValueError(f"L2: weights of shape {w.shape} for an image of shape {self.dims} (an [H, W] or flat array of its size)")
        if y.size != n:
            raise ValueError(f"L2: {y.size} observations for an image of shape {self.dims}")
        if not np.all(np.isfinite(w)):
            raise ValueError("L2: the weights must be finite")
        if np.any(w < 0):
            raise ValueError("L2: the weights must be >= 0 (0 marks an unobserved pixel)")
        if not np.all(np.isfinite(y)):
            raise ValueError("L2: b must be finite where weights are given (mark a bad pixel with weight 0, not with NaN)")
        self.weights = w.reshape(self.dims)
        self._yw = np.ascontiguousarray(np.stack([y.reshape(self.dims), self.weights]), dtype=np.float32)      # [2][H][W]: what y_dev points to
        self._yw_dev = {}

    def _buffer(self):
        """The [2][H][W] device buffer of the weighted term, built once (per device) and kept alive by this object."""
        key = _dev.device(None)
        if key not in self._yw_dev:
            self._yw_dev[key] = _dev.to_dev(self._yw, key)
        return self._yw_dev[key]

    def grad_lipschitz(self):
        """``L_f = sigma * max(w) * ||Op||^2`` with ``||Op|| <= sum |h|`` for a convolution and the factor 1 for a mask (entries in [0, 1]), the
        identity or no operator; ``max(w) = 1`` without weights.  Host arithmetic, no GPU."""
        if self._spectral is not None:      # sigma max_k A_k, A the folded |G|^2
            return self.sigma * self._amax
        if isinstance(self.Op, MultiCoilFourierSampling):      # sigma max M^2 max_p sum_c |S_c(p)|^2
            return self.sigma * self.Op.norm_bound()
        if isinstance(self.Op, Radon):      # ||A||^2 <= max(A 1) max(A^T 1)
            return self.sigma * (float(np.max(self.weights)) if self.weights is not None else 1.0) * self.Op.norm_bound()
        op2 = float(np.abs(np.asarray(self.Op.h, dtype=np.float64)).sum()) ** 2 if isinstance(self.Op, (Convolve2D, PSF)) else 1.0
        wmax = float(np.max(self.weights)) if self.weights is not None else 1.0
        return self.sigma * wmax * op2

    # -- descriptors ---------------------------------------------------------------------
    def descriptor(self):
        """As the data term f of the sampler."""
        if self._spectral is not None:
            tab = self._spectral_buffer() if torch.cuda.is_available() else self._spectral["tab"]
            return {"data_kind": _capi.DATA_SPECTRAL, "sigma_f": self.sigma, "y": tab}
        if isinstance(self.Op, MultiCoilFourierSampling):
            y = self._sense_buffer() if torch.cuda.is_available() else self._sense
            return {"data_kind": _capi.DATA_SENSE, "sigma_f": self.sigma, "y": y, "n_coils": self.Op.n_coils}
        if isinstance(self.Op, Radon):
            if self.weights is not None:
                yw = self._buffer() if torch.cuda.is_available() else self._yw
                return {"data_kind": _capi.DATA_WL2_RADON, "sigma_f": self.sigma, "y": yw, **self.Op.descriptor()}
            return {"data_kind": _capi.DATA_RADON, "sigma_f": self.sigma, "y": self._sino, **self.Op.descriptor()}
        if self.weights is not None:
            yw = self._buffer() if torch.cuda.is_available() else self._yw      # (without a device: the host array, for whoever only reads the description)
            if isinstance(self.Op, PSF):
                return {"data_kind": _capi.DATA_WL2_PSF, "sigma_f": self.sigma, "y": yw, **self.Op.descriptor()}
            if isinstance(self.Op, Convolve2D):
                return {"data_kind": _capi.DATA_WL2_BLUR, "sigma_f": self.sigma, "y": yw, "h": self.Op.h, "offset": self.Op.offset}
            return {"data_kind": _capi.DATA_WL2_IDENTITY, "sigma_f": self.sigma, "y": yw}
        if self.Op is None or isinstance(self.Op, Identity):
            if self.b is None:
                raise NotImplementedError("L2 without b as a data term: use it as the prior instead")
            return {"data_kind": _capi.DATA_IDENTITY, "sigma_f": self.sigma, "y": self.b}
        if isinstance(self.Op, PSF):
            return {"data_kind": _capi.DATA_PSF, "sigma_f": self.sigma, "y": self.b, **self.Op.descriptor()}
        if isinstance(self.Op, Convolve2D):
            return {"data_kind": _capi.DATA_BLUR, "sigma_f": self.sigma, "y": self.b, "h": self.Op.h,
                    "offset": self.Op.offset}
        if isinstance(self.Op, Diagonal):
            return {"data_kind": _capi.DATA_MASK, "sigma_f": self.sigma, "y": self.b, "mask": self.Op.d}
        raise NotImplementedError(f"no device functor for L2 with Op of type {type(self.Op).__name__}")

    def prior_descriptor(self):
        """As the prior g = sigma/2 ||x||^2 (closed-form prox)."""
        if self.Op is not None or self.b is not None:
            raise NotImplementedError("only L2(sigma=...) without Op/b can act as the prior")
        return _with_box({"prior_kind": _capi.PRIOR_L2, "prior_sigma": self.sigma}, self.bounds)

    def _problem(self):
        if self._prob is None:
            if self.dims is None:
                raise ValueError("L2 needs `dims` (image shape) when Op does not carry it")
            self._prob = _Problem(self.dims, data=self.descriptor())
        return self._prob

    # -- protocol ------------------------------------------------------------------------
    def __call__(self, x):
        if self.Op is None and self.b is None:       # pure quadratic prior sigma/2 ||x||^2
            xt = _dev.to_dev(x).reshape(1, -1)
            _, g = _Problem((1, xt.shape[1]), prior=self.prior_descriptor()).energies(xt)
            return float(g[0])
        f, _ = self._problem().energies(x)
        return float(f[0]) if f.numel() == 1 else (f if isinstance(x, torch.Tensor) else f.cpu().numpy())

    def grad(self, x):
        return self._problem().eval(x, 0.0, -1.0, 0.0, 0.0)

    def prox(self, x, tau):
        """``(I + tau*sigma*Op^T Op)^{-1}(x + tau*sigma*Op^T b)`` (pyproximal.L2.prox; in-repo twin algs.py:224-256).
        With a blur operator: ``niter`` warm-started CG iterations on the GPU (lmc_l2_prox)."""
        if self.bounds is not None:
            return _box_prox(self, x, tau)
        if self._spectral is not None:      # closed form between the two column transforms (lmc_l2_prox ignores niter, warm and the workspace)
            prob = self._problem()
            xt = _dev.to_dev(x, prob.device)
            out = torch.empty_like(xt)
            with torch.cuda.device(prob.device):
                _dev.run(xt, "lmc_l2_prox", C.byref(prob.c), _dev.ptr(xt), _dev.ptr(out), xt.numel() // (self.dims[0] * self.dims[1]), float(tau), 0, 0, None)
            return _dev.like_input(out, x)
        if isinstance(self.Op, PSF):
            raise NotImplementedError("L2.prox with a large PSF: the implicit step (I + tau sigma Op^T Op)^{-1} is not built for it (lmc_l2_prox refuses it)")
        if isinstance(self.Op, MultiCoilFourierSampling):
            raise NotImplementedError("L2.prox with MultiCoilFourierSampling: the implicit step (I + tau sigma A^H A)^{-1} is diagonal in neither the pixel nor "
                                      "the Fourier basis and is not built (lmc_l2_prox refuses it)")
        if isinstance(self.Op, Radon):
            raise NotImplementedError("L2.prox with Radon: the implicit step (I + tau sigma A^T A)^{-1} is not built for it (lmc_l2_prox refuses it)")
        if self.weights is not None:
            raise NotImplementedError("L2.prox with weights: the implicit step (I + tau sigma Op^T W Op)^{-1} is not built (lmc_l2_prox refuses it)")
        if self.Op is None and self.b is None:
            return x / (1.0 + tau * self.sigma)
        prob = self._problem()
        n = self.dims[0] * self.dims[1]
        xt = _dev.to_dev(x, prob.device)
        n_img = xt.numel() // n
        lib = _dev.lib()
        if self.warm and self._x0 is not None and self._x0.numel() == xt.numel():
            out, warm = self._x0.clone(), 1
        else:
            out, warm = torch.empty_like(xt), 0
        nbytes = lib.lmc_l2_prox_workspace_bytes(n_img, self.dims[0], self.dims[1])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xt.device)
        with torch.cuda.device(prob.device):
            _capi.check(lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(xt), _dev.ptr(out), n_img, float(tau), int(self.niter),
                                        warm, _dev.ptr(ws), _dev.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        if self.warm:
            self._x0 = out.clone()
        return _dev.like_input(out.reshape(xt.shape), x)


class Poisson(ProxOperator):
    r"""Poisson likelihood of photon-limited imaging, ``b_p ~ Poisson((Op x)_p + background_p)`` (build extension; the reference has no such term --
    ``LMC_DATA_POISSON_*`` in include/lmc_atomi.h is its definition): ``f(x) = sigma * sum_p phi_p((Op x)_p)`` with, for ``u >= 0``,
    ``phi(u) = (u + beta) - y + y log(y / (u + beta))`` -- the generalised Kullback-Leibler divergence, the negative log-likelihood up to a constant --
    and for ``u < 0`` its second-order Taylor extension at 0, ``phi(0) + phi'(0) u + y u^2 / (2 beta^2)``.  The extension makes ``f`` convex and C^1
    everywhere with a Lipschitz gradient (:meth:`grad_lipschitz`), which MYULA needs: its iterates live near the positive orthant, not in it.

    ``Op``: :class:`Convolve2D`, :class:`Diagonal` or :class:`Identity` (``dims``: the image shape where neither ``Op`` nor a 2-D ``b`` carries it);
    ``b``: the counts (>= 0, finite; they need not be integers); ``background``: a
    positive scalar or an ``[H, W]`` array (dark current, known sky); ``sigma = 1`` is the true likelihood.  A pixel with ``b_p = 0`` has a linear ``phi``,
    unbounded below as ``u -> -inf``: USE THE MODEL WITH A POSITIVITY CONSTRAINT on the prior, e.g. ``TV(dims, ..., bounds=(0, inf))``.

    As ``proxf`` of :class:`MYULASampler` / :func:`MoreauYosidaUnadjustedLangevin`, :class:`SKROCKSampler` / :func:`StabilisedLangevin` and
    :func:`EstimatePriorWeight`, with the priors none / L2 / L1 / closed forms / TV (either form, any ``niter``, ``bounds``); the term enters the fused step
    of the full-width pipeline (isotropic TV with 10 dual iterations, W > 128, separable blur or pointwise operator) and of the LDS-tiled kernel everywhere
    else.  MYMALA, ULPDA, ``prox`` (no closed implicit step), ``TV(rtol > 0)``, ``TV(warm=True)``, the block-Haar :class:`WaveletL1` and a forced kernel variant other
    than 'auto' / 'tile' / 'pipe' raise ``NotImplementedError``."""

    def __init__(self, Op, b, background, sigma=1.0, dims=None):
        super().__init__(Op, True)
        if isinstance(Op, Radon):      # emission tomography: counts and background live on the sinogram (LMC_DATA_POISSON_RADON)
            self.dims = Op.dims
            y = _sino_plane(Op, b, "Poisson", "b")
            if not np.all(np.isfinite(y)) or np.any(y < 0):
                raise ValueError("Poisson: the counts b must be finite and >= 0")
            beta = _sino_plane(Op, background, "Poisson", "background", scalar=True)
            if not np.all(np.isfinite(beta)) or np.any(beta <= 0):
                raise ValueError("Poisson: the background must be finite and > 0 (a scalar or an array of the sinogram's shape)")
            self.b, self.background = y, beta
            self.sigma = float(sigma)
            self._yb = np.ascontiguousarray(np.stack([y, beta]), dtype=np.float32)      # [2][n_angles][n_det]: what y_dev points to
            self._yb_dev = {}
            self._prob = None
            return
        if not isinstance(Op, (Convolve2D, PSF, Diagonal, Identity)):
            raise NotImplementedError(f"no device functor for Poisson with Op of type {type(Op).__name__} (Convolve2D, PSF, Diagonal, Identity or Radon)")
        y = _host(b).astype(np.float64)
        # the image shape: `dims`, else the operator's, else that of an [H, W] array of counts or background
        for cand in (dims, getattr(Op, "dims", None), y.shape if y.ndim == 2 else None, np.shape(background) if np.ndim(background) == 2 else None):
            if cand is not None:
                self.dims = (int(cand[0]), int(cand[1]))
                break
        else:
            raise ValueError("Poisson: image shape unknown (Op carries none and b is flat): pass dims=(ny, nx)")
        if y.size != self.dims[0] * self.dims[1]:
            raise ValueError(f"Poisson: {y.size} counts for an image of shape {self.dims}")
        y = y.reshape(self.dims)
        if not np.all(np.isfinite(y)) or np.any(y < 0):
            raise ValueError("Poisson: the counts b must be finite and >= 0")
        beta = _host(background).astype(np.float64)
        if beta.ndim != 0 and beta.size != y.size:
            raise ValueError(f"Poisson: the background must be a scalar or an array of the image's shape {self.dims} (got {beta.shape})")
        beta = np.full(self.dims, float(beta)) if beta.ndim == 0 else beta.reshape(self.dims)
        if not np.all(np.isfinite(beta)) or np.any(beta <= 0):
            raise ValueError("Poisson: the background must be finite and > 0 (a scalar or an [H, W] array)")
        self.b, self.background = y, beta
        self.sigma = float(sigma)
        self._yb = np.ascontiguousarray(np.stack([y, beta]), dtype=np.float32)      # [2][H][W]: what y_dev points to
        self._yb_dev = {}
        self._prob = None

    def _buffer(self):
        """The [2][H][W] device buffer, built once (per device) and kept alive by this object; a problem on another device takes its own copy."""
        key = _dev.device(None)
        if key not in self._yb_dev:
            self._yb_dev[key] = _dev.to_dev(self._yb, key)
        return self._yb_dev[key]

    def descriptor(self):
        yb = self._buffer() if torch.cuda.is_available() else self._yb      # (without a device: the host array, for whoever only reads the description)
        if isinstance(self.Op, Radon):
            return {"data_kind": _capi.DATA_POISSON_RADON, "sigma_f": self.sigma, "y": yb, **self.Op.descriptor()}
        if isinstance(self.Op, PSF):
            return {"data_kind": _capi.DATA_POISSON_PSF, "sigma_f": self.sigma, "y": yb, **self.Op.descriptor()}
        if isinstance(self.Op, Convolve2D):
            return {"data_kind": _capi.DATA_POISSON_BLUR, "sigma_f": self.sigma, "y": yb, "h": self.Op.h, "offset": self.Op.offset}
        if isinstance(self.Op, Diagonal):
            return {"data_kind": _capi.DATA_POISSON_MASK, "sigma_f": self.sigma, "y": yb, "mask": self.Op.d}
        return {"data_kind": _capi.DATA_POISSON_IDENTITY, "sigma_f": self.sigma, "y": yb}

    def grad_lipschitz(self):
        """``L_f = sigma * max(b / background^2) * ||Op||^2`` with ``||Op|| <= sum |h|`` for a convolution and the factor 1 for a mask (entries in [0, 1])
        or the identity.  Host arithmetic, no GPU."""
        if isinstance(self.Op, Radon):      # ||A||^2 <= max(A 1) max(A^T 1)
            return self.sigma * float(np.max(self.b / self.background ** 2)) * self.Op.norm_bound()
        op2 = float(np.abs(np.asarray(self.Op.h, dtype=np.float64)).sum()) ** 2 if isinstance(self.Op, (Convolve2D, PSF)) else 1.0
        return self.sigma * float(np.max(self.b / self.background ** 2)) * op2

    def _problem(self):
        if self._prob is None:
            self._prob = _Problem(self.dims, data=self.descriptor())
        return self._prob

    def __call__(self, x):
        f, _ = self._problem().energies(x)
        return float(f[0]) if f.numel() == 1 else (f if isinstance(x, torch.Tensor) else f.cpu().numpy())

    def grad(self, x):
        return self._problem().eval(x, 0.0, -1.0, 0.0, 0.0)

    def prox(self, x, tau):
        raise NotImplementedError("Poisson.prox: the implicit step of the Poisson likelihood has no closed form (lmc_l2_prox refuses it)")


class HuberLoss(ProxOperator):
    r"""Huber loss of the residual: robust deconvolution with outliers at unknown positions -- impulse noise, cosmic rays, hot or saturated pixels (build
    extension; the reference has no such term -- ``LMC_DATA_HUBER_*`` in include/lmc_atomi.h is its definition).  With ``r = (Op x)_p - b_p``:
    ``f(x) = sigma * sum_p h_delta_p(r_p)``, ``h_delta(r) = r^2 / 2`` for ``|r| <= delta`` and ``delta (|r| - delta / 2)`` beyond, so
    ``grad f = sigma Op^T clamp(Op x - b, -delta, delta)``: the clamp acts on the residual before the adjoint.  (The name ``Huber`` is the prior factory.)

    ``Op``: :class:`Convolve2D`, :class:`Identity` or :class:`PSF` (``dims``: the image shape where neither ``Op`` nor a 2-D ``b`` or ``delta`` carries it);
    ``b``: the observation (finite); ``delta``: a scalar or an ``[H, W]`` / flat array of thresholds in ``[0, +inf]`` -- ``+inf`` is the plain Gaussian
    term at that pixel, ``0`` an unobserved pixel, so a binary mask on a blur is ``delta = 0`` there (``Diagonal`` is refused).  f is convex and C^1 with
    ``L_f = sigma ||Op||^2``.

    As ``proxf`` of :class:`MYULASampler` / :func:`MoreauYosidaUnadjustedLangevin`, :class:`MYMALASampler` (not with ``PSF``), :class:`SKROCKSampler` /
    :func:`StabilisedLangevin` and :func:`EstimatePriorWeight`, with the priors and ``bounds`` of ``L2(weights=...)``.  ``prox``, ULPDA, ``Diagonal``,
    the Fourier-domain operators, ``TV(rtol > 0)``, ``TV(warm=True)``, the block-Haar :class:`WaveletL1` and a forced kernel variant other than 'auto' /
    'tile' / 'pipe' raise ``NotImplementedError``."""

    def __init__(self, Op, b, delta, sigma=1.0, dims=None):
        super().__init__(Op, True)
        if isinstance(Op, Diagonal):
            raise NotImplementedError("HuberLoss with Op = Diagonal: there is no Huber mask kind -- a binary mask on a blur is delta = 0 at the masked pixels")
        if isinstance(Op, (FourierSampling, PeriodicConvolve2D)):
            raise NotImplementedError(f"HuberLoss with Op of type {type(Op).__name__}: the Huber loss of a Fourier-domain residual is not built")
        if isinstance(Op, Radon):      # robust tomography: observation and thresholds live on the sinogram (LMC_DATA_HUBER_RADON)
            self.dims = Op.dims
            y = _sino_plane(Op, b, "HuberLoss", "b")
            if not np.all(np.isfinite(y)):
                raise ValueError("HuberLoss: b must be finite (mark a bad bin with delta = 0, not with NaN)")
            d = _sino_plane(Op, delta, "HuberLoss", "delta", scalar=True)
            if np.any(np.isnan(d)) or np.any(d < 0):
                raise ValueError("HuberLoss: delta must be >= 0 and not NaN (0 marks an unobserved bin, +inf the plain quadratic term)")
            self.b, self.delta = y, d
            self.sigma = float(sigma)
            self._yd = np.ascontiguousarray(np.stack([y, d]), dtype=np.float32)      # [2][n_angles][n_det]: what y_dev points to
            self._yd_dev = {}
            self._prob = None
            return
        if not isinstance(Op, (Convolve2D, PSF, Identity)):
            raise NotImplementedError(f"no device functor for HuberLoss with Op of type {type(Op).__name__} (Convolve2D, PSF, Identity or Radon)")
        y = _host(b).astype(np.float64)
        d = _host(delta).astype(np.float64)
        # the image shape: `dims`, else the operator's, else that of an [H, W] array of observations or thresholds
        for cand in (dims, getattr(Op, "dims", None), y.shape if y.ndim == 2 else None, d.shape if d.ndim == 2 else None):
            if cand is not None:
                self.dims = (int(cand[0]), int(cand[1]))
                break
        else:
            raise ValueError("HuberLoss: image shape unknown (Op carries none, b and delta are flat): pass dims=(ny, nx)")
        n = self.dims[0] * self.dims[1]
        if y.size != n:
            raise ValueError(f"HuberLoss: {y.size} observations for an image of shape {self.dims}")
        if not np.all(np.isfinite(y)):
            raise ValueError("HuberLoss: b must be finite (mark a bad pixel with delta = 0, not with NaN)")
        if d.ndim != 0 and (d.size != n or d.ndim not in (1, 2) or (d.ndim == 2 and d.shape != self.dims)):
            raise ValueError(f"HuberLoss: delta of shape {d.shape} for an image of shape {self.dims} (a scalar, or an [H, W] or flat array of its size)")
        if np.any(np.isnan(d)) or np.any(d < 0):
            raise ValueError("HuberLoss: delta must be >= 0 and not NaN (0 marks an unobserved pixel, +inf the plain quadratic term)")
        self.b = y.reshape(self.dims)
        self.delta = np.full(self.dims, float(d)) if d.ndim == 0 else d.reshape(self.dims)
        self.sigma = float(sigma)
        self._yd = np.ascontiguousarray(np.stack([self.b, self.delta]), dtype=np.float32)      # [2][H][W]: what y_dev points to
        self._yd_dev = {}
        self._prob = None

    def _buffer(self):
        """The [2][H][W] device buffer, built once (per device) and kept alive by this object; a problem on another device takes its own copy."""
        key = _dev.device(None)
        if key not in self._yd_dev:
            self._yd_dev[key] = _dev.to_dev(self._yd, key)
        return self._yd_dev[key]

    def descriptor(self):
        yd = self._buffer() if torch.cuda.is_available() else self._yd      # (without a device: the host array, for whoever only reads the description)
        if isinstance(self.Op, Radon):
            return {"data_kind": _capi.DATA_HUBER_RADON, "sigma_f": self.sigma, "y": yd, **self.Op.descriptor()}
        if isinstance(self.Op, PSF):
            return {"data_kind": _capi.DATA_HUBER_PSF, "sigma_f": self.sigma, "y": yd, **self.Op.descriptor()}
        if isinstance(self.Op, Convolve2D):
            return {"data_kind": _capi.DATA_HUBER_BLUR, "sigma_f": self.sigma, "y": yd, "h": self.Op.h, "offset": self.Op.offset}
        return {"data_kind": _capi.DATA_HUBER_IDENTITY, "sigma_f": self.sigma, "y": yd}

    def grad_lipschitz(self):
        """``L_f = sigma * ||Op||^2`` (the clamp is 1-Lipschitz: the bound of the plain term) with ``||Op|| <= sum |h|`` for a convolution and 1 for the
        identity.  Host arithmetic, no GPU."""
        if isinstance(self.Op, Radon):      # ||A||^2 <= max(A 1) max(A^T 1)
            return self.sigma * self.Op.norm_bound()
        op2 = float(np.abs(np.asarray(self.Op.h, dtype=np.float64)).sum()) ** 2 if isinstance(self.Op, (Convolve2D, PSF)) else 1.0
        return self.sigma * op2

    def _problem(self):
        if self._prob is None:
            self._prob = _Problem(self.dims, data=self.descriptor())
        return self._prob

    def __call__(self, x):
        f, _ = self._problem().energies(x)
        return float(f[0]) if f.numel() == 1 else (f if isinstance(x, torch.Tensor) else f.cpu().numpy())

    def grad(self, x):
        return self._problem().eval(x, 0.0, -1.0, 0.0, 0.0)

    def prox(self, x, tau):
        raise NotImplementedError("HuberLoss.prox: the implicit step of the Huber loss under an operator is not built (lmc_l2_prox refuses it)")


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _sino_plane(op, a, who, what, scalar=False):
    """``a`` as a float64 ``[n_angles, n_det]`` plane of the sinogram of the Radon operator ``op`` (``scalar``: a scalar fills it); ``ValueError`` for
    any other size."""
    v = _host(a).astype(np.float64)
    if scalar and v.ndim == 0:
        return np.full(op.sino_shape, float(v))
    if v.size != op.sino_shape[0] * op.sino_shape[1] or (v.ndim >= 2 and v.shape != op.sino_shape):
        raise ValueError(f"{who} with Radon: {what} of shape {v.shape} for a sinogram of shape {op.sino_shape} ([n_angles, n_det] or flat)")
    return v.reshape(op.sino_shape)


class L1(ProxOperator):
    """``sigma ||x||_1`` -- drop-in for ``pyproximal.L1(sigma=tau)`` (prox_lmc_deconv.py:119)."""

    def __init__(self, sigma=1.0, dims=None, bounds=None):
        super().__init__(None, False)
        self.sigma = float(sigma)
        self.dims = dims
        self.bounds = check_bounds(bounds)        # sigma ||x||_1 + the indicator of [lo, hi]: prox = clip(soft threshold)

    def prior_descriptor(self):
        return _with_box({"prior_kind": _capi.PRIOR_L1, "prior_sigma": self.sigma}, self.bounds)

    def __call__(self, x):
        xt = _dev.to_dev(x).reshape(1, -1)
        p = _Problem((1, xt.shape[1]), prior=self.prior_descriptor())
        _, g = p.energies(xt)
        return float(g[0])

    def prox(self, x, tau):
        if self.bounds is not None:
            return _box_prox(self, x, tau)
        xt = _dev.to_dev(x)
        out = torch.empty_like(xt)
        par = np.asarray([self.sigma * float(tau)], dtype=np.float32)
        _dev.run(xt, "lmc_prox_elementwise", _capi.EPROX_LAPLACE, _dev.ptr(xt), _dev.ptr(out), xt.numel(),
                                                    _dev.fptr(par), 1)
        return _dev.like_input(out, x)

    def proxdual(self, x, tau):
        """Clip to [-sigma, sigma] (projection onto the dual ball)."""
        xt = _dev.to_dev(x)
        out = torch.empty_like(xt)
        par = np.asarray([self.sigma], dtype=np.float32)
        _dev.run(xt, "lmc_prox_elementwise", _capi.EPROX_UNIFORM, _dev.ptr(xt), _dev.ptr(out), xt.numel(),
                                                    _dev.fptr(par), 1)
        return _dev.like_input(out, x)


class L21(ProxOperator):
    """``sigma * sum_pixels ||(v_row, v_col)||_2`` on stacked fields of length 2n -- drop-in for
    ``pyproximal.L21(ndim=2, sigma=tau)`` (prox_lmc_deconv.py:116)."""

    def __init__(self, ndim=2, sigma=1.0):
        if ndim != 2:
            raise NotImplementedError("ndim=2 only (the reference's configuration)")
        super().__init__(None, False)
        self.ndim = ndim
        self.sigma = float(sigma)

    def __call__(self, x):
        xt = _dev.to_dev(x).reshape(2, -1)
        return self.sigma * float(torch.sqrt((xt.double() ** 2).sum(0)).sum())

    def proxdual(self, x, tau):
        xt = _dev.to_dev(x)
        n2 = xt.shape[-1]
        if n2 % 2:
            raise ValueError("stacked field must have even length")
        out = torch.empty_like(xt)
        _dev.run(xt, "lmc_dual_project", _dev.ptr(xt), _dev.ptr(out), xt.numel() // n2, 1, n2 // 2,
                                                self.sigma, 1)
        return _dev.like_input(out, x)

    def prox(self, x, tau):
        """Moreau identity with the dual projection: prox_{tau g}(x) = x - proj_{tau*sigma}(x)."""
        xt = _dev.to_dev(x)
        n2 = xt.shape[-1]
        out = torch.empty_like(xt)
        _dev.run(xt, "lmc_dual_project", _dev.ptr(xt), _dev.ptr(out), xt.numel() // n2, 1, n2 // 2,
                                                self.sigma * float(tau), 1)
        return _dev.like_input(xt - out, x)


class TV(ProxOperator):
    """``sigma * TV_iso(x)`` -- drop-in for ``pyproximal.TV(dims=img.shape, sigma=tau, niter=niter_tv)``
    (prox_lmc_deconv.py:122).  ``prox`` runs ``niter`` fast-gradient-projection dual iterations fully
    on chip.

    ``isotropic=False`` (build extension; pyproximal's ``TV`` has no anisotropic form): ``sigma * (||d_r x||_1 + ||d_c x||_1)``, the same
    dual iteration with the dual clipped to [-1, 1] per component instead of projected onto the pixel-norm ball.  Fixed count only:
    ``rtol > 0`` and ``warm=True`` raise ``NotImplementedError``.

    Deviations from upstream, both named in DESIGN section 4:

    * ``rtol``: pyproximal's per-image early exit on the relative change of the primal objective (its default 1e-4, which the
      reference's call does not override).  Default here: 0 = off, every image runs ``niter`` dual iterations in ONE fused launch (against
      the reference as configured the trajectory differs by 1.5e-4 rel-L2 and the posterior mean by 8e-5).
      ``rtol > 0`` reproduces the reference's configured behaviour -- every image leaves in the pass upstream's loop leaves it in:
      decided on the device without synchronisation where the full-width pipeline covers the image (every width above 128 columns, rows
      of any alignment, ``niter <= 60``: every chain runs with the pass count it left in at the previous call, the launch leaves the primal
      objectives of its iterates behind, chains whose prediction was wrong run again; images wider than 512 columns run as column strips
      that add their shares of every objective), pass by pass elsewhere -- one launch per loop pass plus one for its objective and a host
      read after every pass; landing there without having asked for it (``W <= 128``) raises a ``RuntimeWarning`` once per process, and
      ``exit_path='passes'`` forces that path silently.
    * ``lagged_output``: whether upstream's truncated iterate after ``niter`` loop passes reflects ``niter`` or ``niter - 1`` dual
      updates depends on the loop bound of the un-pinned upstream version; ``False`` (default) = ``niter`` updates,
      ``True`` = ``niter - 1`` (one pipeline stage fewer).
    * ``warm`` (build extension, MYULA samplers only): carry the projected dual from one MYULA iteration to the next, ``niter``
      in {1, 2, 3} updates per MYULA iteration ("K in {1,3} warm-dual").
    * ``bounds=(lo, hi)`` (build extension; either form of the prior): ``g(x) = sigma TV(x) +`` the indicator of ``lo <= x <= hi``.  ``prox`` is Beck and
      Teboulle's constrained fast gradient projection -- the primal iterate is projected onto the box inside every dual iteration, which converges to the
      prox of the sum (clipping the unconstrained prox afterwards does not).  Infinite ends are allowed.  ``__call__`` keeps returning ``sigma TV(x)``.
      Fixed count only: ``rtol > 0`` and ``warm=True`` raise ``NotImplementedError``."""

    def __init__(self, dims, sigma=1.0, niter=10, rtol=0.0, step=0.125, momentum="unlocbox", lagged_output=False, warm=False, exit_path="auto",
                 isotropic=True, bounds=None):
        super().__init__(None, False)
        self.isotropic = bool(isotropic)
        self.bounds = check_bounds(bounds)
        if self.bounds is not None and float(rtol) > 0.0:
            raise NotImplementedError("TV(bounds=...) has no early exit: rtol must be 0 (every image runs niter dual iterations)")
        if self.bounds is not None and warm:
            raise NotImplementedError("TV(bounds=...) has no warm-started dual: warm must be False")
        if self.bounds is not None and int(niter) < 1:
            raise ValueError("TV(bounds=...): the projection runs inside the dual iterations, niter must be >= 1")
        if not self.isotropic and float(rtol) > 0.0:
            raise NotImplementedError("TV(isotropic=False) has no early exit: rtol must be 0 (every image runs niter dual iterations)")
        if not self.isotropic and warm:
            raise NotImplementedError("TV(isotropic=False) has no warm-started dual: warm must be False")
        self.dims = (int(dims[0]), int(dims[1]))
        self.sigma = float(sigma)
        self.niter = int(niter)
        self.rtol = float(rtol)
        self.exit_path = {"auto": 0, "device": 0, "passes": 1}[exit_path]
        self.step = float(step)
        self.momentum = momentum
        self.lagged_output = bool(lagged_output)
        self.warm = bool(warm)
        self._prob = None

    def prior_descriptor(self):
        return _with_box({"prior_kind": _capi.PRIOR_TV_ISO if self.isotropic else _capi.PRIOR_TV_ANISO, "prior_sigma": self.sigma, "tv_niter": self.niter,
                          "tv_step": self.step, "tv_betas": fgp_betas(self.niter, self.momentum),
                          "tv_lagged_output": self.lagged_output, "tv_warm": self.warm, "tv_rtol": self.rtol, "tv_exit_path": self.exit_path}, self.bounds)

    def _problem(self):
        if self._prob is None:
            self._prob = _Problem(self.dims, prior=self.prior_descriptor())
        return self._prob

    def __call__(self, x):
        _, g = self._problem().energies(x)
        return float(g[0]) if g.numel() == 1 else (g if isinstance(x, torch.Tensor) else g.cpu().numpy())

    def prox(self, x, tau):
        return self._problem().eval(x, 0.0, 0.0, 1.0, float(tau))


class ElementwiseProx(ProxOperator):
    """A separable prior given by one of the closed-form proxes of the reference's ``prox.py`` (prox.py:18-85; used inside its samplers at
    prox_lmc.py:106,115 as ``prox.prox_laplace(theta, lamda * alpha)``): ``prox(x, tau) = prox_<kind>(x, *params)`` pixel by pixel, with the
    parameters listed in ``scaled`` multiplied by ``tau`` first.  As ``proxg`` of the MYULA samplers it is evaluated INSIDE the fused step
    kernel (``LMC_PRIOR_EPROX``: row-streaming, register-block and tiled kernels); stand-alone it is ``lmc_prox_elementwise``.

    ``kind``: 'laplace' | 'uncentered_laplace' | 'gaussian' | 'gen_gaussian_4_3' | 'gen_gaussian_3_2' | 'gen_gaussian_3' | 'gen_gaussian_4' |
    'huber' | 'smoothed_laplace' | 'exp' | 'gamma' | 'chi' | 'uniform' | 'triangular' | 'laplace_conj' (parameter order as in prox.py).
    The value g(x) is not defined for every family (the reference only ever uses their proxes): ``__call__`` returns 0."""

    KINDS = {"laplace": (_capi.EPROX_LAPLACE, 1), "uncentered_laplace": (_capi.EPROX_UNCENTERED_LAPLACE, 2), "gaussian": (_capi.EPROX_GAUSSIAN, 1),
             "gen_gaussian_4_3": (_capi.EPROX_GEN_GAUSSIAN_4_3, 1), "gen_gaussian_3_2": (_capi.EPROX_GEN_GAUSSIAN_3_2, 1),
             "gen_gaussian_3": (_capi.EPROX_GEN_GAUSSIAN_3, 1), "gen_gaussian_4": (_capi.EPROX_GEN_GAUSSIAN_4, 1), "huber": (_capi.EPROX_HUBER, 2),
             "smoothed_laplace": (_capi.EPROX_SMOOTHED_LAPLACE, 1), "exp": (_capi.EPROX_EXP, 1), "gamma": (_capi.EPROX_GAMMA, 2),
             "chi": (_capi.EPROX_CHI, 1), "uniform": (_capi.EPROX_UNIFORM, 1), "triangular": (_capi.EPROX_TRIANGULAR, 2),
             "laplace_conj": (_capi.EPROX_LAPLACE_CONJ, 1)}

    def __init__(self, kind, *params, scaled=(), bounds=None):
        super().__init__(None, False)
        self.bounds = check_bounds(bounds)        # g + the indicator of [lo, hi]: prox = clip(closed form)
        if kind not in self.KINDS:
            raise ValueError(f"unknown closed-form prox {kind!r}")
        self.kind = kind
        self.code, n = self.KINDS[kind]
        if len(params) != n:
            raise ValueError(f"prox_{kind} takes {n} parameter(s)")
        self.params = tuple(float(v) for v in params)
        self.scaled = tuple(int(i) for i in scaled)
        if any(i < 0 or i >= n for i in self.scaled):
            raise ValueError("scaled: indices of the parameters that are multiplied by tau")
        _capi.check_eprox_params(self.code, self.params)      # weights >= 0; 0 is the identity

    def _scaled_params(self, tau):
        return [v * float(tau) if i in self.scaled else v for i, v in enumerate(self.params)]

    def prior_descriptor(self):
        p = self.params + (0.0,) * (2 - len(self.params))
        return _with_box({"prior_kind": _capi.PRIOR_EPROX, "eprox_kind": self.code, "eprox_p0": p[0], "eprox_p1": p[1],
                          "eprox_scale_mask": sum(1 << i for i in self.scaled)}, self.bounds)

    def __call__(self, x):
        return 0.0

    def prox(self, x, tau):
        if self.bounds is not None:
            _capi.check_eprox_params(self.code, self._scaled_params(tau))
            return _box_prox(self, x, tau)
        xt = _dev.to_dev(x)
        out = torch.empty_like(xt)
        _capi.check_eprox_params(self.code, self._scaled_params(tau))
        par = np.asarray(self._scaled_params(tau), dtype=np.float32)
        _dev.run(xt, "lmc_prox_elementwise", self.code, _dev.ptr(xt), _dev.ptr(out), xt.numel(), _dev.fptr(par), par.size)
        return _dev.like_input(out, x)


def Laplace(lam, bounds=None):
    """``lam * ||x||_1`` through ``prox_laplace(x, tau * lam)`` (prox.py:18; prox_lmc.py:106)."""
    return ElementwiseProx("laplace", lam, scaled=(0,), bounds=bounds)


def UncenteredLaplace(lam, mu, bounds=None):
    return ElementwiseProx("uncentered_laplace", lam, mu, scaled=(0,), bounds=bounds)       # prox.py:22


def Gaussian(lam, bounds=None):
    return ElementwiseProx("gaussian", lam, scaled=(0,), bounds=bounds)                     # prox.py:26: x / (2 tau lam + 1)


def GenGaussian(p, lam, bounds=None):
    """``lam * |x|^p``, p in {4/3, 3/2, 3, 4} (prox.py:30-41)."""
    names = {4 / 3: "gen_gaussian_4_3", 3 / 2: "gen_gaussian_3_2", 3: "gen_gaussian_3", 4: "gen_gaussian_4"}
    if p not in names:
        raise ValueError("p must be one of 4/3, 3/2, 3, 4")
    return ElementwiseProx(names[p], lam, scaled=(0,), bounds=bounds)


def Huber(gamma, tau, bounds=None):
    return ElementwiseProx("huber", gamma, tau, scaled=(1,), bounds=bounds)                 # prox.py:44: tau is the prox weight


def SmoothedLaplace(lam, bounds=None):
    return ElementwiseProx("smoothed_laplace", lam, scaled=(0,), bounds=bounds)             # prox.py:52


class Box(ProxOperator):
    """The indicator of ``lo <= x <= hi`` alone (build extension): ``prox`` is the projection onto the box, whatever ``tau``.  As ``proxg`` of the MYULA
    samplers it is the constrained sampler of Durmus, Moulines and Pereyra with a flat prior: the Moreau-Yosida envelope of the indicator pulls the
    iterates towards the box, it does not keep them inside.  ``__call__`` returns 0 (the value inside the box)."""

    def __init__(self, lo, hi):
        super().__init__(None, False)
        self.bounds = check_bounds((lo, hi))

    def prior_descriptor(self):
        return _with_box({"prior_kind": _capi.PRIOR_NONE}, self.bounds)

    def __call__(self, x):
        return 0.0

    def prox(self, x, tau):
        return _box_prox(self, x, tau)


class WaveletL1(ProxOperator):
    """``sigma * || detail coefficients of an orthonormal wavelet transform of x ||_1`` (build-specified; the reference has no wavelet code);
    ``prox`` = W^T soft(W x, tau*sigma), exact.

    ``wavelet='haar'`` with ``levels=3`` (the default) is the prior of BASELINE config 5, ``LMC_PRIOR_HAAR_L1``: the 3-level Haar transform on
    independent 8 x 8 blocks, with the kernels it has always had.  ``'haar'`` with another level count and ``'db1'`` .. ``'db4'`` with any are
    ``LMC_PRIOR_WAVELET_L1`` (include/lmc_atomi.h is its definition): the periodic transform of the Daubechies extremal-phase filter with p vanishing
    moments over ``levels`` levels (1 .. 8); the sides must be multiples of ``2^levels`` and the coarsest level must hold the filter,
    ``min(H, W) >> (levels - 1) >= 2p``.  ``'db1'`` is the Haar filter through the general transform.  As ``proxg`` of MYULA, MYMALA, SK-ROCK and
    :func:`EstimatePriorWeight`, with every data term; ``bounds``, ULPDA and array-valued ``epsg`` raise ``NotImplementedError``."""

    def __init__(self, dims, sigma=1.0, levels=3, bounds=None, wavelet="haar"):
        super().__init__(None, False)
        if bounds is not None:
            raise NotImplementedError("WaveletL1 takes no bounds: the prior is not separable in the pixels, so clipping its prox is not the prox of the sum")
        self.dims = (int(dims[0]), int(dims[1]))
        self.wavelet = wavelet
        self.p, self.levels = _capi.check_wavelet(self.dims, wavelet, levels)
        self.block_haar = wavelet == "haar" and self.levels == 3
        self.sigma = float(sigma)
        self._prob = None

    def prior_descriptor(self):
        if self.block_haar:
            return {"prior_kind": _capi.PRIOR_HAAR_L1, "prior_sigma": self.sigma}
        return {"prior_kind": _capi.PRIOR_WAVELET_L1, "prior_sigma": self.sigma, "wavelet_p": self.p, "wavelet_levels": self.levels}

    def __call__(self, x):
        if self._prob is None:
            self._prob = _Problem(self.dims, prior=self.prior_descriptor())
        _, g = self._prob.energies(x)
        return float(g[0]) if g.numel() == 1 else (g if isinstance(x, torch.Tensor) else g.cpu().numpy())

    def prox(self, x, tau):
        xt = _dev.to_dev(x)
        out = torch.empty_like(xt)
        n = self.dims[0] * self.dims[1]
        if self.block_haar:
            _dev.run(xt, "lmc_haar_l1_prox", _dev.ptr(xt), _dev.ptr(out), xt.numel() // n, self.dims[0], self.dims[1],
                                                    self.sigma * float(tau))
        else:
            _dev.run(xt, "lmc_wavelet_l1_prox", _dev.ptr(xt), _dev.ptr(out), xt.numel() // n, self.dims[0], self.dims[1], self.p, self.levels,
                                                       self.sigma * float(tau))
        return _dev.like_input(out, x)


class VectorialTV(ProxOperator):
    """``sigma * VTV(x)`` on a multi-channel image ``x[ch, H, W]``: ``VTV(x) = sum_pixels sqrt(sum_ch (d_r x_ch)^2 + (d_c x_ch)^2)``, ONE gradient norm per
    pixel over all channels (Blomgren-Chan / Bresson-Chan; build-specified, ``LMC_PRIOR_VTV`` in include/lmc_atomi.h is its definition).  The channels of an
    RGB photograph, a Bayer mosaic, a dual-energy CT pair share their edges; this prior says so, and running the channels as unrelated grey problems
    under :class:`TV` samples another posterior.  ``prox`` is ``niter`` (1 .. 64) fast-gradient-projection dual iterations from the zero dual with the
    projection weight shared by the channels of a pixel; ``n_channels=1`` is :class:`TV`.  ``bounds=(lo, hi)``: the constrained form, as ``TV(bounds=...)``.

    ``prox(x, tau)`` and ``__call__(x)`` take ``[nch, H, W]``, a batch ``[nch, n, H, W]`` (channel-major: each channel's images contiguous) or a flat array of
    one of those sizes; ``prox`` returns the shape it was given, ``__call__`` one value per multi-channel image.  As ``proxg`` of
    :class:`MultichannelMYULASampler` and of :func:`MoreauYosidaUnadjustedLangevin` (which routes to it); every other sampler raises
    ``NotImplementedError``."""

    def __init__(self, dims, n_channels, sigma=1.0, niter=10, step=0.125, momentum="unlocbox", bounds=None):
        super().__init__(None, False)
        self.dims = (int(dims[0]), int(dims[1]))
        if self.dims[0] < 1 or self.dims[1] < 1:
            raise ValueError(f"dims must be a pair of positive sizes (got {dims!r})")
        self.n_channels = int(n_channels)
        if not 1 <= self.n_channels <= _capi.MAX_CHANNELS:
            raise ValueError(f"n_channels must be in 1 .. {_capi.MAX_CHANNELS} (got {n_channels})")
        self.niter = int(niter)
        if not 1 <= self.niter <= _capi.MAX_TV_ITERS:
            raise ValueError(f"niter must be in 1 .. {_capi.MAX_TV_ITERS} (got {niter})")
        self.bounds = check_bounds(bounds)
        self.sigma = float(sigma)
        if not self.sigma >= 0.0:
            raise ValueError(f"sigma must be >= 0 (got {sigma})")
        self.step = float(step)
        if not self.step > 0.0:
            raise ValueError(f"step must be > 0 (got {step})")
        self.momentum = momentum
        self._betas = fgp_betas(self.niter, momentum)

    def prior_descriptor(self):
        return _with_box({"prior_kind": _capi.PRIOR_VTV, "prior_sigma": self.sigma, "tv_niter": self.niter, "tv_step": self.step, "tv_betas": self._betas,
                          "n_channels": self.n_channels}, self.bounds)

    def _batch(self, x):
        """The number of multi-channel images in ``x``; ``ValueError`` for a shape that is none of ``[nch, H, W]``, ``[nch, n, H, W]`` or flat of those sizes."""
        shape = tuple(x.shape) if isinstance(x, torch.Tensor) else tuple(np.shape(x))
        one = self.n_channels * self.dims[0] * self.dims[1]
        size = int(np.prod(shape)) if shape else 1
        ok = (len(shape) == 1 and size and size % one == 0) or shape == (self.n_channels,) + self.dims or \
             (len(shape) == 4 and shape[0] == self.n_channels and shape[1] >= 1 and shape[2:] == self.dims)
        if not ok:
            raise ValueError(f"operand of shape {shape} is neither [{self.n_channels}, {self.dims[0]}, {self.dims[1]}], nor a batch [{self.n_channels}, n, "
                             f"{self.dims[0]}, {self.dims[1]}], nor flat of one of those sizes")
        return size // one

    def __call__(self, x):
        n = self._batch(x)
        xt = _dev.to_dev(x)
        g = torch.empty(n, dtype=torch.float64, device=xt.device)
        _dev.run(xt, "lmc_vtv_value", _dev.ptr(xt), _dev.ptr(g), n, self.n_channels, n * self.dims[0] * self.dims[1], self.dims[0], self.dims[1])
        g = g * self.sigma
        return float(g[0]) if n == 1 else (g if isinstance(x, torch.Tensor) else g.cpu().numpy())

    def prox(self, x, tau):
        n = self._batch(x)
        xt = _dev.to_dev(x)
        out = torch.empty_like(xt)
        lo, hi = self.bounds if self.bounds is not None else (0.0, 0.0)
        _dev.run(xt, "lmc_vtv_prox", _dev.ptr(xt), _dev.ptr(out), n, self.n_channels, n * self.dims[0] * self.dims[1], self.dims[0], self.dims[1],
                 self.sigma * float(tau), self.niter, self.step, _dev.fptr(self._betas), 1 if self.bounds is not None else 0, lo, hi)
        return _dev.like_input(out, x)


class TGV(ProxOperator):
    """``sigma * TGV2(x)``: total generalised variation of order two (Bredies, Kunisch and Pock 2010; build-specified, ``LMC_PRIOR_TGV`` in
    include/lmc_atomi.h is its definition),

        ``g(x) = sigma * min_w ( sum |grad x - w|_2 + alpha0 * sum |E w|_F )``

    with ``E`` the symmetrised derivative of the field ``w``.  An intensity ramp costs nothing, where :class:`TV` charges its full variation and samples
    it as terraces.  ``prox`` is ``niter`` (1 .. 256) Chambolle-Pock primal-dual iterations with one step ``step`` for both sides (None: 1 / sqrt(12);
    ``12 step^2 > 1`` raises ``ValueError``) from ``u = x``, ``w = 0`` and zero duals, run on chip by ``tgv_prox_kernel``.  The count is fixed and the
    result is the truncated iterate, the same kind of truncation as ``TV(niter=10)``: the iteration converges sublinearly -- on a 32 x 48 two-facet affine
    image with noise of sd 10 at ``tau * sigma = 5`` the distance to the converged prox, relative to ``|prox - x|``, is 0.14, 0.085, 0.048, 0.032, 0.021
    after 10, 20, 40, 80, 160 iterations (float64 prototype; the TV prox moves the clean ramp by 5.9 grey levels, this one by 0.46).
    ``bounds=(lo, hi)``: ``g +`` the indicator of the box; the primal iterate is clipped inside every iteration, the exact prox of its quadratic plus the
    indicator (clipping afterwards gives another point).

    ``prox(x, tau)`` takes a flat image, ``[H, W]`` or a batch ``[n, H, W]`` (or flat of that size) and returns the shape it was given;
    ``prox(x, tau, return_w=True)`` also returns the auxiliary field ``w`` as ``[..., 2, H, W]`` (row component first).  ``__call__`` raises
    ``NotImplementedError``: the value is a minimisation over ``w`` and is not built, so the samplers report ``energy_g = 0`` for it.  As ``proxg`` of
    MYULA and SK-ROCK (:class:`MYULASampler`, :class:`SKROCKSampler` and their drivers) with every data term, the box (MYULA), the accumulators and
    sharding; MYMALA, ULPDA, :func:`EstimatePriorWeight` and array-valued ``epsg`` raise ``NotImplementedError``."""

    def __init__(self, dims, sigma=1.0, alpha0=2.0, niter=40, bounds=None, step=None):
        super().__init__(None, False)
        self.dims = (int(dims[0]), int(dims[1]))
        if self.dims[0] < 1 or self.dims[1] < 1:
            raise ValueError(f"dims must be a pair of positive sizes (got {dims!r})")
        self.sigma = float(sigma)
        if not self.sigma >= 0.0 or not np.isfinite(self.sigma):
            raise ValueError(f"sigma must be finite and >= 0 (got {sigma})")
        self.alpha0 = float(alpha0)
        if not self.alpha0 > 0.0 or not np.isfinite(self.alpha0):
            raise ValueError(f"alpha0 must be finite and > 0 (got {alpha0})")
        self.niter = int(niter)
        if not 1 <= self.niter <= _capi.MAX_TGV_ITERS:
            raise ValueError(f"niter must be in 1 .. {_capi.MAX_TGV_ITERS} (got {niter})")
        self.bounds = check_bounds(bounds)
        self.step = 0.0 if step is None else float(step)      # 0: the library's default, 1 / sqrt(12)
        if step is not None and (not self.step > 0.0 or not np.isfinite(self.step) or 12.0 * self.step * self.step > 1.0 + 1e-6):
            raise ValueError(f"step must be > 0 with 12 step^2 <= 1 (got {step}): the primal-dual iteration needs step^2 ||K||^2 <= 1")

    def prior_descriptor(self):
        return _with_box({"prior_kind": _capi.PRIOR_TGV, "prior_sigma": self.sigma, "tgv_niter": self.niter, "tgv_alpha0": self.alpha0,
                          "tgv_step": self.step}, self.bounds)

    def __call__(self, x):
        raise NotImplementedError("TGV has no value: g(x) is a minimisation over the auxiliary field w and is not built (its prox is; the samplers report "
                                  "energy_g = 0 for this prior)")

    def prox(self, x, tau, return_w=False):
        xt = _dev.to_dev(x)
        n = self.dims[0] * self.dims[1]
        if xt.numel() == 0 or xt.numel() % n:
            raise ValueError(f"operand of shape {tuple(xt.shape)} is not a batch of {self.dims} images")
        n_img = xt.numel() // n
        out = torch.empty_like(xt)
        w = torch.empty((n_img, 2) + self.dims, dtype=torch.float32, device=xt.device) if return_w else None
        lo, hi = self.bounds if self.bounds is not None else (0.0, 0.0)
        _dev.run(xt, "lmc_tgv_prox", _dev.ptr(xt), _dev.ptr(out), _dev.ptr(w), n_img, self.dims[0], self.dims[1], self.sigma * float(tau), self.alpha0,
                 self.niter, self.step, 1 if self.bounds is not None else 0, lo, hi)
        u = _dev.like_input(out, x)
        if not return_w:
            return u
        lead = tuple(xt.shape[:-2]) if xt.dim() >= 2 and tuple(xt.shape[-2:]) == self.dims else ((n_img,) if n_img > 1 else ())
        w = w.reshape(lead + (2,) + self.dims)
        return u, (w if isinstance(x, torch.Tensor) else w.cpu().numpy())


class L2_ncvx_tv(ProxOperator):
    r"""Non-log-concave data term -- drop-in for the reference's own class ``algs.L2_ncvx_tv`` (algs.py:22-291):
    ``f(x) = sigma/2 ||Op x - b||^2 - lamda * env_gamma(g)(Op2 x)``, same constructor arguments.

    Built on the GPU, both isotropic branches used by prox_lmc_deconv.py:106-113:
    * MC-TV (``Op2 = Gradient``): value (algs.py:173-190), gradient (:270-291,
      ``sigma Op^T(Op x - b) - lamda * Op2^T( Op2 x / max(|Op2 x|, gamma) )``) fused into the sampler step, and the implicit
      ``prox`` (:201-267; also inside ULPDA, prox_lmc_deconv.py:478-487);
    * ME-TV (``Op2 = None``): value and gradient ``sigma Op^T(Op x - b) - lamda (x - prox_{gamma TV}(x))/gamma`` (:282), the inner
      TV prox with ``niter`` (= niter_l2 = 50) dual iterations chained exactly through HBM-resident dual state in chunks of 8.
    ``prox`` (:201-267) is built for both (ME-TV pre-step :221-223).  Round 2: the anisotropic MC-TV branches too (``isotropic=False``
    with ``Op2 = Gradient``: :218-219, :278-279 -- the weight of a difference is 1 / max(|that difference|, gamma)).  Round 3: anisotropic
    ME-TV (``isotropic=False``, ``Op2 = None``: a 1-D TV over the flattened image, :170) as plain coverage -- one pass over the images per
    dual iteration of its inner prox, not fused (no model of the reference's driver uses it).
    """

    def __init__(self, dims, Op=None, Op2=None, b=None, q=None, sigma=1., alpha=1., lamda=1., gamma=.5, qgrad=True,
                 isotropic=False, niter=10, rtol=1e-4, x0=None, warm=True, densesolver=None, kwargs_solver=None, lagged_output=False):
        super().__init__(Op, True)
        from .operators import Gradient
        if q is not None:
            raise NotImplementedError("q (linear term) has no device functor")
        if Op2 is not None and not isinstance(Op2, Gradient):
            raise NotImplementedError("Op2 must be a Gradient (MC-TV) or None (ME-TV)")
        from .operators import Identity
        if not isinstance(Op, (Convolve2D, Diagonal, Identity)) or b is None:
            raise NotImplementedError("Op must be a Convolve2D (prox_lmc_deconv.py:106), a Diagonal mask or an Identity, and b given")
        self.dims = (int(dims[0]), int(dims[1]))
        self.Op2 = Op2
        self.b = b
        self.sigma, self.lamda, self.gamma = float(sigma), float(lamda), float(gamma)
        self.isotropic = isotropic
        self.niter = niter
        self.warm = warm
        # the reference hands rtol to its inner TV(dims, 1., niter, rtol) (algs.py:169): that prox is only used by the ME-TV branch, where
        # every image leaves the inner prox in the pass upstream's loop leaves it in (lmc_problem.ncvx_rtol; rtol = 0: always niter updates)
        self.rtol = float(rtol)
        self.lagged_output = bool(lagged_output)
        self._prob = None

    def descriptor(self):
        if isinstance(self.Op, Diagonal):
            base = {"data_kind": _capi.DATA_MASK, "sigma_f": self.sigma, "y": self.b, "mask": self.Op.d}
        elif not isinstance(self.Op, Convolve2D):     # Identity (denoising)
            base = {"data_kind": _capi.DATA_IDENTITY, "sigma_f": self.sigma, "y": self.b}
        else:
            base = {"data_kind": _capi.DATA_BLUR, "sigma_f": self.sigma, "y": self.b, "h": self.Op.h, "offset": self.Op.offset}
        if self.Op2 is None:       # ME-TV: isotropic (2-D TV, algs.py:169) or the 1-D TV of the flattened image (algs.py:170)
            kind = _capi.NCVX_ME_TV if self.isotropic else _capi.NCVX_ME_TV_ANISO
        else:
            kind = _capi.NCVX_MC_TV if self.isotropic else _capi.NCVX_MC_TV_ANISO
        return {**base, "ncvx_kind": kind,
                "ncvx_lambda": self.lamda, "ncvx_gamma": self.gamma, "ncvx_niter": int(self.niter),
                "ncvx_rtol": self.rtol if self.Op2 is None else 0.0,
                "tv_lagged_output": self.lagged_output}

    def _problem(self):
        if self._prob is None:
            self._prob = _Problem(self.dims, data=self.descriptor())
        return self._prob

    def __call__(self, x):
        f, _ = self._problem().energies(x)
        return float(f[0]) if f.numel() == 1 else (f if isinstance(x, torch.Tensor) else f.cpu().numpy())

    def grad(self, x):
        return self._problem().eval(x, 0.0, -1.0, 0.0, 0.0)

    def prox(self, x, tau):
        """``L2_ncvx_tv.prox`` (algs.py:201-267), MC-TV branch: ``v <- x + tau*lamda*Op2^T(Op2 x / max(|Op2 x|, gamma))`` then
        ``(I + tau sigma Op^T Op)^{-1}(v + tau sigma Op^T b)`` by ``niter`` warm-started CG iterations (lmc_l2_prox).  Unlike
        the reference (which adds the first term into its argument in place, :217) the input is left untouched."""
        prob = self._problem()
        n = self.dims[0] * self.dims[1]
        xt = _dev.to_dev(x, prob.device)
        n_img = xt.numel() // n
        lib = _dev.lib()
        x0 = getattr(self, "_x0", None)
        if self.warm and x0 is not None and x0.numel() == xt.numel():
            out, warm = x0.clone(), 1
        else:
            out, warm = torch.empty_like(xt), 0
        ws = torch.empty(lib.lmc_l2_prox_workspace_bytes(n_img, self.dims[0], self.dims[1]), dtype=torch.uint8, device=xt.device)
        with torch.cuda.device(prob.device):
            _capi.check(lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(xt), _dev.ptr(out), n_img, float(tau), int(self.niter), warm,
                                        _dev.ptr(ws), _dev.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        if self.warm:
            self._x0 = out.clone()
        return _dev.like_input(out.reshape(xt.shape), x)
