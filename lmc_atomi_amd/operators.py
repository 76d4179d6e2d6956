"""Linear operators with the pylops protocol the reference's samplers consume
(``.matvec`` / ``.rmatvec`` / ``.shape`` / ``.H`` / ``*`` / ``@`` / ``.dtype`` / ``.explicit``:
algs.py:159-162,174,213,427,436-437), computed by HIP kernels through the C ABI.

Inputs may be numpy arrays (uploaded, result returned as numpy) or torch tensors in HBM
(result stays in HBM).  Flat vectors of length n (or batches ``[..., n]``) as in the reference.
"""
from __future__ import annotations

import numpy as np

from . import _capi, _dev


class LinearOperator:
    explicit = False
    dtype = np.dtype(np.float32)

    def __init__(self, shape):
        self.shape = tuple(int(s) for s in shape)

    @property
    def H(self):
        return _Adjoint(self)

    adjoint = lambda self: self.H  # noqa: E731  (pylops spelling used at prox.py:15)

    def __mul__(self, x):
        return self.matvec(x)

    __matmul__ = __mul__

    def __rmul__(self, a):
        return _Scaled(self, float(a))

    def _batch(self, x, n_in):
        """-> (fp32 HBM tensor [n_img, n_in], n_img, leading batch shape).  Accepts a flat vector
        ``(n_in,)``, a batch ``(..., n_in)`` or image-shaped ``(..., H, W)`` operands."""
        t = _dev.to_dev(x)
        if t.shape[-1] == n_in:
            lead = tuple(t.shape[:-1])
        elif t.ndim >= 2 and hasattr(self, "dims") and tuple(t.shape[-2:]) == self.dims and n_in == self.dims[0] * self.dims[1]:
            lead = tuple(t.shape[:-2])
        else:
            raise ValueError(f"operand of shape {tuple(t.shape)} does not match operator input size {n_in}")
        return t.reshape(-1, n_in), int(t.numel() // n_in), lead


class _Adjoint(LinearOperator):
    def __init__(self, op):
        super().__init__((op.shape[1], op.shape[0]))
        self.op = op

    def matvec(self, x):
        return self.op.rmatvec(x)

    def rmatvec(self, y):
        return self.op.matvec(y)


class _Scaled(LinearOperator):
    def __init__(self, op, a):
        super().__init__(op.shape)
        self.op, self.a = op, a

    def matvec(self, x):
        return self.a * self.op.matvec(x)

    def rmatvec(self, y):
        return self.a * self.op.rmatvec(y)


class Convolve2D(LinearOperator):
    """Zero-padded "same" convolution with origin ``offset`` -- drop-in for
    ``pylops.signalprocessing.Convolve2D((ny, nx), h=h, offset=(oy, ox))`` as constructed at
    prox_lmc_deconv.py:55-69.  ``matvec`` = H x, ``rmatvec`` = H^T x (lmc_blur)."""

    def __init__(self, dims, h, offset=None, dtype=None):
        self.dims = (int(dims[0]), int(dims[1]))
        n = self.dims[0] * self.dims[1]
        super().__init__((n, n))
        self.h = np.ascontiguousarray(np.asarray(h, dtype=np.float32))
        if self.h.ndim != 2:
            raise ValueError("h must be 2-D")
        kh, kw = self.h.shape
        if kh > _capi.MAX_BLUR or kw > _capi.MAX_BLUR:
            raise ValueError(f"kernels larger than {_capi.MAX_BLUR}x{_capi.MAX_BLUR} are not supported")
        self.offset = (kh // 2, kw // 2) if offset is None else (int(offset[0]), int(offset[1]))

    def _apply(self, x, adjoint):
        import torch
        t, n_img, _ = self._batch(x, self.shape[1])
        out = torch.empty_like(t)
        kh, kw = self.h.shape
        _dev.run(t, "lmc_blur", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1],
                                        _dev.fptr(self.h), kh, kw, self.offset[0], self.offset[1],
                                        1 if adjoint else 0)
        return _dev.like_input(out.reshape(tuple(np.shape(x))), x)

    def matvec(self, x):
        return self._apply(x, False)

    def rmatvec(self, y):
        return self._apply(y, True)


class PSF(LinearOperator):
    """The same zero-padded "same" convolution with origin ``offset`` for a realistic point-spread function: ``h`` of 1 .. 33 taps in each direction
    (a Gaussian of sigma = 5 px at +-3 sigma, a motion blur, an Airy pattern), any origin inside it (default: the centre tap).  ``matvec`` = H x,
    ``rmatvec`` = H^T x (lmc_psf_apply).  ``separable``: None -- two 1-D passes where ``h`` is an outer product to a fraction of float32 rounding
    (``lmc_psf_separable``: :attr:`factors`), the general 2-D form elsewhere; True -- require the two-pass form (``ValueError`` where ``h`` is no outer
    product); False -- always the general form.  As ``Op`` of :class:`L2` (with or without ``weights``) and :class:`Poisson` in MYULA, SK-ROCK and
    :func:`EstimatePriorWeight`; MYMALA, ULPDA, ``L2.prox``, the non-convex terms, ``TV(rtol > 0)`` and ``TV(warm=True)`` raise ``NotImplementedError``.
    :class:`Convolve2D` (up to 9 x 9, inside the fused step kernels) is unchanged."""

    def __init__(self, dims, h, offset=None, separable=None):
        self.dims = (int(dims[0]), int(dims[1]))
        n = self.dims[0] * self.dims[1]
        super().__init__((n, n))
        h64 = np.asarray(h, dtype=np.float64)
        if h64.ndim != 2:
            raise ValueError("h must be 2-D")
        kh, kw = h64.shape
        if not (1 <= kh <= _capi.MAX_PSF and 1 <= kw <= _capi.MAX_PSF):
            raise ValueError(f"PSF of {kh}x{kw} taps: 1 .. {_capi.MAX_PSF} in each direction are supported")
        if not np.all(np.isfinite(h64)):
            raise ValueError("the taps of the PSF must be finite")
        self.h = np.ascontiguousarray(h64, dtype=np.float32)
        self.offset = (kh // 2, kw // 2) if offset is None else (int(offset[0]), int(offset[1]))
        if not (0 <= self.offset[0] < kh and 0 <= self.offset[1] < kw):
            raise ValueError(f"offset {self.offset} outside the {kh}x{kw} kernel")
        if separable not in (None, True, False):
            raise ValueError("separable must be None (auto), True (require) or False (forbid)")
        self.separable = separable
        self._factors = None
        if separable is not False:      # the library's own test (host only: no device needed)
            u, v = np.zeros(kh, dtype=np.float32), np.zeros(kw, dtype=np.float32)
            rc = _capi.load().lmc_psf_separable(_dev.fptr(self.h), kh, kw, _dev.fptr(u), _dev.fptr(v))
            if rc < 0:
                _capi.check(rc)
            if rc == 1:
                self._factors = (u, v)
            elif separable:
                raise ValueError("separable=True, but h is no outer product u v^T to 2^-22 of every tap (lmc_psf_separable)")

    @property
    def factors(self):
        """``(u, v)`` with ``h = u v^T`` where the two-pass form runs, else ``None``."""
        return self._factors

    def _mode(self):
        return 2 if self.separable is False else (1 if self.separable else 0)

    def descriptor(self):
        """The operator's part of a data-term descriptor (``lmc_problem.psf_*``)."""
        return {"h": self.h, "offset": self.offset, "psf_separable": self._mode()}

    def _apply(self, x, adjoint):
        import torch
        t, n_img, _ = self._batch(x, self.shape[1])
        out = torch.empty_like(t)
        kh, kw = self.h.shape
        _dev.run(t, "lmc_psf_apply", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1],
                 _dev.fptr(self.h), kh, kw, self.offset[0], self.offset[1], 1 if adjoint else 0, self._mode())
        return _dev.like_input(out.reshape(tuple(np.shape(x))), x)

    def matvec(self, x):
        return self._apply(x, False)

    def rmatvec(self, y):
        return self._apply(y, True)


class Radon(LinearOperator):
    """Parallel-beam Radon operator for transmission CT and emission tomography (PET / SPECT) -- build extension; ``LMC_DATA_RADON`` in
    include/lmc_atomi.h is its definition: the pixel-driven projector with linear interpolation on a detector of ``n_det`` unit bins, pixel ``(i, j)``
    at ``t = X_j cos(theta) + Y_i sin(theta) + (n_det - 1) / 2`` giving ``max(0, 1 - |t - d|)`` of its value to bin ``d``.  ``angles``: 1 .. 1024
    finite angles in radians (rounded to float32 once: those values are the angles); ``n_det``: 1 .. 4096, default ``ceil(hypot(H, W)) + 2`` -- every
    pixel then keeps its full weight at every angle; a detector narrower than the image truncates.  ``matvec``: images ``[..., H*W]`` or
    ``[..., H, W]`` -> sinograms ``[..., n_angles*n_det]``; ``rmatvec`` / ``.H``: the exact adjoint (``lmc_radon_apply``).  As ``Op`` of :class:`L2`
    (with or without ``weights``), :class:`Poisson` and :class:`HuberLoss` (``b``, ``weights``, ``background``, ``delta`` of the sinogram's size) in
    MYULA, SK-ROCK and :func:`EstimatePriorWeight` with every prior and ``bounds=`` a problem without a data term takes; MYMALA, ULPDA, the terms'
    ``prox``, the non-convex terms, ``TV(rtol > 0)`` and ``TV(warm=True)`` raise ``NotImplementedError``."""

    def __init__(self, dims, angles, n_det=None):
        try:
            self.dims = (int(dims[0]), int(dims[1]))
        except (TypeError, ValueError, IndexError):
            raise ValueError(f"dims must be a pair (H, W) (got {dims!r})") from None
        H, W = self.dims
        if H < 1 or W < 1 or max(H, W) > _capi.MAX_RADON_SIDE:
            raise ValueError(f"Radon: image sides must be in 1 .. {_capi.MAX_RADON_SIDE} (got {H} x {W})")
        a = np.atleast_1d(np.asarray(angles, dtype=np.float64))
        if a.ndim != 1 or not 1 <= a.size <= _capi.MAX_RADON_ANGLES:
            raise ValueError(f"Radon: angles must be a 1-D array of 1 .. {_capi.MAX_RADON_ANGLES} angles (got shape {np.shape(angles)})")
        with np.errstate(over="ignore"):
            a32 = np.ascontiguousarray(a, dtype=np.float32)
        if not np.all(np.isfinite(a)) or not np.all(np.isfinite(a32)):
            raise ValueError("Radon: the angles must be finite (as float32)")
        self.angles = a32
        n_det = int(np.ceil(np.hypot(H, W))) + 2 if n_det is None else int(n_det)
        if not 1 <= n_det <= _capi.MAX_RADON_DET:
            raise ValueError(f"Radon: n_det must be in 1 .. {_capi.MAX_RADON_DET} (got {n_det})")
        self.n_det = n_det
        self.n_angles = int(self.angles.size)
        self.sino_shape = (self.n_angles, self.n_det)
        super().__init__((self.n_angles * self.n_det, H * W))
        self._bound = None

    def descriptor(self):
        """The operator's part of a data-term descriptor (``lmc_problem``: kh = n_angles, kw = n_det, h_host = the angles)."""
        return {"angles": self.angles, "n_det": self.n_det}

    def tables(self):
        """``(ax, by)``, float32 ``[n_angles, W]`` and ``[n_angles, H]``, as the kernels read them (``lmc_radon_tables``: host only)."""
        H, W = self.dims
        ax = np.empty((self.n_angles, W), dtype=np.float32)
        by = np.empty((self.n_angles, H), dtype=np.float32)
        _capi.check(_capi.load().lmc_radon_tables(_dev.fptr(self.angles), self.n_angles, self.n_det, H, W, _dev.fptr(ax), _dev.fptr(by)))
        return ax, by

    def norm_bound(self):
        """``max(A 1) * max(A^T 1) >= ||A||^2`` (A has no negative entry), from the tables in float64 on the host; cached."""
        if self._bound is None:
            ax, by = self.tables()
            stride = self.n_det + 1                                # bin n_det of every angle takes what falls off the detector
            rows = np.zeros(self.n_angles * stride)
            cols = np.zeros(self.dims)
            base = (np.arange(self.n_angles) * stride)[:, None]
            for i in range(self.dims[0]):
                t = (ax + by[:, i:i + 1]).astype(np.float64)      # (the float32 sum IS t)
                f = np.floor(t)
                w1 = t - f
                for d, w in ((f, 1.0 - w1), (f + 1.0, w1)):
                    ok = (d >= 0) & (d < self.n_det)
                    w = np.where(ok, w, 0.0)
                    rows += np.bincount((base + np.where(ok, d, self.n_det).astype(np.int64)).ravel(), weights=w.ravel(), minlength=rows.size)
                    cols[i] += w.sum(0)
            self._bound = float(rows.reshape(self.n_angles, stride)[:, :-1].max() * cols.max())
        return self._bound

    def _apply(self, x, adjoint):
        import torch
        n_in, n_out = (self.shape[0], self.shape[1]) if adjoint else (self.shape[1], self.shape[0])
        t = _dev.to_dev(x)
        if t.shape[-1] == n_in:
            lead = tuple(t.shape[:-1])
        elif t.ndim >= 2 and tuple(t.shape[-2:]) == (self.sino_shape if adjoint else self.dims):
            lead = tuple(t.shape[:-2])
        else:
            raise ValueError(f"operand of shape {tuple(t.shape)} does not match operator input size {n_in}")
        t = t.reshape(-1, n_in)
        n_img = int(t.shape[0])
        out = torch.empty((n_img, n_out), dtype=torch.float32, device=t.device)
        _dev.run(t, "lmc_radon_apply", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1], _dev.fptr(self.angles), self.n_angles, self.n_det,
                 1 if adjoint else 0)
        return _dev.like_input(out.reshape(lead + (n_out,)), x)

    def matvec(self, x):
        return self._apply(x, False)

    def rmatvec(self, y):
        return self._apply(y, True)


class Gradient(LinearOperator):
    """Stacked forward differences ``[d_row x; d_col x]`` (zero in the last row / column) --
    drop-in for ``pylops.Gradient(dims, sampling=1, edge=False, kind='forward')``
    (prox_lmc_deconv.py:98).  ``rmatvec`` = -div."""

    def __init__(self, dims, sampling=1.0, edge=False, kind="forward", dtype=None):
        if sampling != 1 or edge or kind != "forward":
            raise NotImplementedError("only sampling=1, edge=False, kind='forward' (the reference's configuration)")
        self.dims = (int(dims[0]), int(dims[1]))
        n = self.dims[0] * self.dims[1]
        super().__init__((2 * n, n))

    def matvec(self, x):
        import torch
        t, n_img, lead = self._batch(x, self.shape[1])
        out = torch.empty((n_img, 2 * self.shape[1]), dtype=torch.float32, device=t.device)
        _dev.run(t, "lmc_gradient", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1])
        return _dev.like_input(out.reshape(lead + (2 * self.shape[1],)), x)

    def rmatvec(self, y):
        import torch
        t = _dev.to_dev(y)
        if t.shape[-1] != self.shape[0]:
            raise ValueError(f"operand of shape {tuple(t.shape)} does not match the stacked field size {self.shape[0]}")
        lead = tuple(t.shape[:-1])
        t = t.reshape(-1, self.shape[0])
        n_img = t.shape[0]
        out = torch.empty((n_img, self.shape[1]), dtype=torch.float32, device=t.device)
        _dev.run(t, "lmc_gradient_adjoint", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1])
        return _dev.like_input(out.reshape(lead + (self.shape[1],)), y)


class Wavelet2D(LinearOperator):
    """The orthonormal periodic wavelet transform of :class:`~lmc_atomi_amd.proximal.WaveletL1` as an operator (``lmc_wavelet_apply``), to look at
    coefficients: ``wavelet`` in 'haar' / 'db1' .. 'db4', ``levels`` in 1 .. 8, the shape rules of ``LMC_PRIOR_WAVELET_L1`` (include/lmc_atomi.h).
    ``matvec`` = W x in Mallat layout -- the approximation at the top-left, the details of level j in the other three quadrants of the
    ``(H >> (j-1), W >> (j-1))`` corner; ``rmatvec`` / ``.H`` = W^T = W^-1."""

    def __init__(self, dims, wavelet="db2", levels=3):
        self.dims = (int(dims[0]), int(dims[1]))
        self.wavelet = wavelet
        self.p, self.levels = _capi.check_wavelet(self.dims, wavelet, levels)
        n = self.dims[0] * self.dims[1]
        super().__init__((n, n))

    def _apply(self, x, inverse):
        import torch
        t, n_img, lead = self._batch(x, self.shape[1])
        out = torch.empty_like(t)
        _dev.run(t, "lmc_wavelet_apply", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1], self.p, self.levels, inverse)
        return _dev.like_input(out.reshape(lead + (self.shape[0],)), x)

    def matvec(self, x):
        return self._apply(x, 0)

    def rmatvec(self, y):
        return self._apply(y, 1)


class Identity(LinearOperator):
    """``pylops.Identity(n)`` (prox_lmc_deconv.py:125)."""

    def __init__(self, n, dtype=None):
        super().__init__((int(n), int(n)))

    def matvec(self, x):
        return x.clone() if hasattr(x, "clone") else np.array(x, copy=True)

    rmatvec = matvec


class Diagonal(LinearOperator):
    """Diagonal (inpainting mask) operator; the data term of BASELINE config 5."""

    def __init__(self, d, dims=None):
        self.d = np.ascontiguousarray(np.asarray(d, dtype=np.float32)).ravel()
        self.dims = None if dims is None else (int(dims[0]), int(dims[1]))
        super().__init__((self.d.size, self.d.size))


def rfft2(x):
    """``numpy.fft.rfft2(x, norm="ortho")`` of real images on the last two axes (``lmc_rfft2``: the LDS transforms of the spectral data term): sides that
    are powers of two in 8 .. 1024, complex64 on the half plane ``[..., H, W // 2 + 1]``.  numpy in, numpy out; a torch tensor in HBM stays there."""
    import torch
    if np.ndim(x) < 2:
        raise ValueError("rfft2 takes images on the last two axes")
    H, W = _capi.check_fft_dims(tuple(x.shape)[-2:])
    t = _dev.to_dev(x)
    n_img = t.numel() // (H * W)
    out = torch.empty(tuple(t.shape[:-1]) + (W // 2 + 1, 2), dtype=torch.float32, device=t.device)
    _dev.run(t, "lmc_rfft2", _dev.ptr(t), _dev.ptr(out), n_img, H, W)
    c = torch.view_as_complex(out)
    return c if isinstance(x, torch.Tensor) else c.cpu().numpy()


def irfft2(c, dims):
    """``numpy.fft.irfft2(c, s=dims, norm="ortho")`` of half-plane spectra ``[..., H, W // 2 + 1]`` (``lmc_irfft2``), float32 images ``[..., H, W]``."""
    import torch
    H, W = _capi.check_fft_dims(dims)
    if np.ndim(c) < 2 or tuple(c.shape)[-2:] != (H, W // 2 + 1):
        raise ValueError(f"irfft2: a spectrum of shape {tuple(np.shape(c))} is not the half plane [..., {H}, {W // 2 + 1}] of {H} x {W} images")
    if isinstance(c, torch.Tensor):
        if not c.is_complex():
            raise ValueError("irfft2 takes a complex spectrum")
        t = torch.view_as_real(c.to(device=_dev.device(c.device if c.is_cuda else None), dtype=torch.complex64).contiguous())
    else:
        a = np.ascontiguousarray(np.asarray(c), dtype=np.complex64)
        t = torch.from_numpy(a.view(np.float32).reshape(a.shape + (2,))).to(_dev.device(None))
    n_img = t.numel() // (2 * H * (W // 2 + 1))
    out = torch.empty(tuple(t.shape[:-3]) + (H, W), dtype=torch.float32, device=t.device)
    _dev.run(t, "lmc_irfft2", _dev.ptr(t), _dev.ptr(out), n_img, H, W)
    return out if isinstance(c, torch.Tensor) else out.cpu().numpy()


def _minus_k(a):
    """``a`` at ``-k = ((-i) mod H, (-j) mod W)``."""
    return np.roll(np.flip(a, (0, 1)), (1, 1), (0, 1))


def spectral_tables(G, b):
    """The ``[11, H, W // 2 + 1]`` float32 planes of ``LMC_DATA_SPECTRAL`` from the full-plane complex gain ``G`` and data ``b`` (``lmc_spectral_tables``:
    host only, folded in float64)."""
    G = np.ascontiguousarray(G, dtype=np.complex128)
    b = np.ascontiguousarray(b, dtype=np.complex128)
    H, W = _capi.check_fft_dims(G.shape)
    out = np.empty((_capi.SPECTRAL_PLANES, H, W // 2 + 1), dtype=np.float32)
    dptr = lambda a: a.view(np.float64).ctypes.data_as(_capi.C.POINTER(_capi.C.c_double))      # noqa: E731
    _capi.check(_capi.load().lmc_spectral_tables(dptr(G), dptr(b), H, W, _dev.fptr(out)))
    return out


class FourierSampling:
    """Observation in Fourier space (build extension; ``LMC_DATA_SPECTRAL`` in include/lmc_atomi.h is its definition): ``y = G * F x + noise`` with F the
    unitary 2-D DFT in numpy's unshifted ``fft2(norm="ortho")`` order and ``G = mask * transfer`` per frequency -- subsampled k-space MRI, gridded
    radio-interferometric visibilities.  ``mask``: real, >= 0, finite, full plane ``[H, W]`` (it need not be Hermitian-symmetric); ``transfer``: an
    optional complex ``[H, W]`` array.  Sides: powers of two in 8 .. 1024.  Use as ``L2(Op=FourierSampling(dims, mask), b=y_complex, sigma=...)``, with
    ``weights=w`` per frequency for ``G sqrt(w)`` and ``b sqrt(w)``: ``grad``, ``__call__``, the closed-form ``prox`` and ``grad_lipschitz``; as
    ``proxf`` of MYULA, SK-ROCK and :func:`EstimatePriorWeight` with every prior and ``bounds=`` a problem without a data term takes.  MYMALA, ULPDA,
    :class:`Poisson`, the non-convex terms, ``TV(rtol > 0)`` and ``TV(warm=True)`` raise ``NotImplementedError``."""

    def __init__(self, dims, mask, transfer=None):
        self.dims = _capi.check_fft_dims(dims)
        m = np.asarray(mask)
        if np.iscomplexobj(m) or m.shape != self.dims:
            raise ValueError(f"FourierSampling: mask must be a real array of the full plane {self.dims} (got shape {m.shape}, dtype {m.dtype})")
        m = m.astype(np.float64)
        if not np.all(np.isfinite(m)) or np.any(m < 0):
            raise ValueError("FourierSampling: the mask must be finite and >= 0")
        self.mask = m
        self.transfer = None
        if transfer is not None:
            t = np.asarray(transfer, dtype=np.complex128)
            if t.shape != self.dims:
                raise ValueError(f"FourierSampling: transfer of shape {t.shape} for the full plane {self.dims}")
            if not np.all(np.isfinite(t)):
                raise ValueError("FourierSampling: the transfer function must be finite")
            self.transfer = t
        n = self.dims[0] * self.dims[1]
        self.shape = (n, n)

    def gain(self):
        """G, complex128 ``[H, W]``."""
        return self.mask.astype(np.complex128) if self.transfer is None else self.mask * self.transfer

    def data(self, b):
        """``b`` as the complex full-plane data; a real ``b`` is refused (k-space measurements are complex)."""
        a = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
        if not np.iscomplexobj(a):
            raise ValueError("L2 with FourierSampling: b must be complex, the measurements on the full plane [H, W]")
        if a.size != self.dims[0] * self.dims[1]:
            raise ValueError(f"L2 with FourierSampling: {a.size} measurements for the full plane {self.dims}")
        a = a.astype(np.complex128).reshape(self.dims)
        if not np.all(np.isfinite(a)):
            raise ValueError("L2 with FourierSampling: b must be finite (drop a frequency with mask 0, not with NaN)")
        return a


class MultiCoilFourierSampling(LinearOperator):
    """Multi-coil (SENSE) MRI acquisition (build extension; ``LMC_DATA_SENSE`` in include/lmc_atomi.h is its definition): coil ``c`` observes
    ``mask * F(maps[c] * x)`` of the real image ``x``, F the unitary 2-D DFT in numpy's unshifted ``fft2(norm="ortho")`` order over the full plane.
    ``maps``: complex ``[n_coils, H, W]`` sensitivity maps, 1 .. 32 coils, finite (rounded to complex64 once: those values are the maps); ``mask``:
    real ``[H, W]``, >= 0, finite, default ones -- a binary sampling mask or sqrt(density weight).  Sides: powers of two in 8 .. 1024.  ``matvec``:
    images ``[..., H*W]`` or ``[..., H, W]`` -> complex64 k-space ``[..., n_coils*H*W]``; ``rmatvec`` / ``.H``: complex k-space (flat or
    ``[..., n_coils, H, W]``) -> ``sum_c Re[conj(maps[c]) F^H(mask * k_c)]``, the adjoint over the reals (``lmc_sense_apply``).  As ``Op`` of
    ``L2(Op, b, sigma)`` with complex ``b`` of shape ``[n_coils, H, W]`` (or flat) in MYULA, SK-ROCK and :func:`EstimatePriorWeight` with every prior
    and ``bounds=`` a problem without a data term takes; MYMALA, ULPDA, the split Gibbs sampler, ``VectorialTV``, ``L2.prox``, ``L2(weights=)``,
    :class:`Poisson`, :class:`HuberLoss`, the non-convex terms, ``TV(rtol > 0)`` and ``TV(warm=True)`` raise ``NotImplementedError``."""

    dtype = np.dtype(np.complex64)

    def __init__(self, dims, maps, mask=None):
        self.dims = _capi.check_fft_dims(dims)
        H, W = self.dims
        s = maps.detach().cpu().numpy() if hasattr(maps, "detach") else np.asarray(maps)
        if s.ndim != 3 or tuple(s.shape[1:]) != self.dims:
            raise ValueError(f"MultiCoilFourierSampling: maps must be a complex array [n_coils, {H}, {W}] (got shape {s.shape})")
        if not 1 <= s.shape[0] <= _capi.MAX_COILS:
            raise ValueError(f"MultiCoilFourierSampling: 1 .. {_capi.MAX_COILS} coils (got {s.shape[0]})")
        with np.errstate(over="ignore"):
            s64 = np.ascontiguousarray(s, dtype=np.complex64)
        if not np.all(np.isfinite(s)) or not np.all(np.isfinite(s64)):
            raise ValueError("MultiCoilFourierSampling: the maps must be finite (as complex64)")
        self.maps = s64
        self.n_coils = int(s64.shape[0])
        m = np.ones(self.dims) if mask is None else (mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask))
        if np.iscomplexobj(m) or m.shape != self.dims:
            raise ValueError(f"MultiCoilFourierSampling: mask must be a real array of the full plane {self.dims} (got shape {m.shape}, dtype {m.dtype})")
        m = m.astype(np.float64)
        with np.errstate(over="ignore"):
            m32 = np.ascontiguousarray(m, dtype=np.float32)
        if not np.all(np.isfinite(m)) or not np.all(np.isfinite(m32)) or np.any(m < 0):
            raise ValueError("MultiCoilFourierSampling: the mask must be finite and >= 0")
        self.mask = m32
        self.kspace_shape = (self.n_coils, H, W)
        super().__init__((self.n_coils * H * W, H * W))
        self._head = np.ascontiguousarray(np.concatenate([self.mask[None], self.maps.view(np.float32).reshape(self.n_coils, H, W, 2)
                                                          .transpose(0, 3, 1, 2).reshape(2 * self.n_coils, H, W)]))
        self._head_dev = {}
        self._bound = None

    def data(self, b):
        """``b`` as the complex64 ``[n_coils, H, W]`` data; a real ``b`` is refused (k-space measurements are complex)."""
        a = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
        if not np.iscomplexobj(a):
            raise ValueError("L2 with MultiCoilFourierSampling: b must be complex, the measurements [n_coils, H, W]")
        if a.size != self.shape[0] or (a.ndim != 1 and tuple(a.shape) != self.kspace_shape):
            raise ValueError(f"L2 with MultiCoilFourierSampling: b of shape {a.shape} for the k-space {self.kspace_shape} (or flat)")
        with np.errstate(over="ignore"):
            a64 = np.ascontiguousarray(a.reshape(self.kspace_shape), dtype=np.complex64)
        if not np.all(np.isfinite(a)) or not np.all(np.isfinite(a64)):
            raise ValueError("L2 with MultiCoilFourierSampling: b must be finite (drop a frequency with mask 0, not with NaN)")
        return a64

    def descriptor(self, b=None):
        """The float32 planes ``y_dev`` points to: ``[1 + 2 n_coils, H, W]`` (mask, Re / Im of every map; what ``lmc_sense_apply`` reads) or, with the
        data ``b``, ``[1 + 4 n_coils, H, W]`` (then Re / Im of every coil's data)."""
        if b is None:
            return self._head
        H, W = self.dims
        d = self.data(b).view(np.float32).reshape(self.n_coils, H, W, 2).transpose(0, 3, 1, 2).reshape(2 * self.n_coils, H, W)
        return np.ascontiguousarray(np.concatenate([self._head, d]))

    def norm_bound(self):
        """``max mask^2 * max_p sum_c |maps[c](p)|^2 >= ||A||^2`` (``lmc_sense_lipschitz``: host only, float64); cached."""
        if self._bound is None:
            v = float(_capi.load().lmc_sense_lipschitz(_dev.fptr(self._head), self.dims[0], self.dims[1], self.n_coils))
            if v < 0:
                _capi.check(int(v))
            self._bound = v
        return self._bound

    def _head_buffer(self, dev):
        if dev not in self._head_dev:
            self._head_dev[dev] = _dev.to_dev(self._head, dev)
        return self._head_dev[dev]

    def matvec(self, x):
        import torch
        t, n_img, lead = self._batch(x, self.shape[1])
        out = torch.empty((n_img, self.shape[0], 2), dtype=torch.float32, device=t.device)
        _dev.run(t, "lmc_sense_apply", _dev.ptr(self._head_buffer(t.device)), _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1], self.n_coils, 0)
        c = torch.view_as_complex(out).reshape(lead + (self.shape[0],))
        return c if isinstance(x, torch.Tensor) else c.cpu().numpy()

    def rmatvec(self, k):
        import torch
        n_in, n_out = self.shape
        if isinstance(k, torch.Tensor):
            if not k.is_complex():
                raise ValueError("MultiCoilFourierSampling.rmatvec takes complex k-space")
            c = k.to(device=_dev.device(k.device if k.is_cuda else None), dtype=torch.complex64).contiguous()
        else:
            a = np.asarray(k)
            if not np.iscomplexobj(a):
                raise ValueError("MultiCoilFourierSampling.rmatvec takes complex k-space")
            dev = _dev.device(None)
            c = torch.from_numpy(np.array(a, dtype=np.complex64, order="C")).to(dev)
        if c.shape[-1] == n_in:
            lead = tuple(c.shape[:-1])
        elif c.ndim >= 3 and tuple(c.shape[-3:]) == self.kspace_shape:
            lead = tuple(c.shape[:-3])
        else:
            raise ValueError(f"operand of shape {tuple(c.shape)} does not match the k-space {self.kspace_shape} (or flat, {n_in})")
        t = torch.view_as_real(c.reshape(-1, n_in))
        n_img = int(t.shape[0])
        out = torch.empty((n_img, n_out), dtype=torch.float32, device=t.device)
        _dev.run(t, "lmc_sense_apply", _dev.ptr(self._head_buffer(t.device)), _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1], self.n_coils, 1)
        out = out.reshape(lead + (n_out,))
        return out if isinstance(k, torch.Tensor) else out.cpu().numpy()


class PeriodicConvolve2D(LinearOperator):
    """Periodic (wrap-around) convolution with a kernel ``h`` of any support up to the image and origin ``offset`` (default: the centre tap):
    ``(H x)[i, j] = sum_ab h[a, b] x[(i - a + oy) mod H, (j - b + ox) mod W]`` -- :class:`Convolve2D` with the borders joined.  In Fourier space the blur
    is a diagonal multiply whatever its support: ``matvec``, ``rmatvec`` and ``.H`` run ``lmc_spectral_filter`` with the unnormalised DFT of the kernel
    wrapped about its origin (``rmatvec``: its conjugate).  Sides: powers of two in 8 .. 1024.  As ``Op`` of ``L2(Op, b_real, sigma)`` it makes the
    descriptor of :class:`FourierSampling` with ``G`` that DFT and ``b = F(observation)``."""

    def __init__(self, dims, h, offset=None):
        self.dims = _capi.check_fft_dims(dims)
        n = self.dims[0] * self.dims[1]
        super().__init__((n, n))
        h64 = np.asarray(h, dtype=np.float64)
        if h64.ndim != 2:
            raise ValueError("h must be 2-D")
        kh, kw = h64.shape
        if kh < 1 or kw < 1 or kh > self.dims[0] or kw > self.dims[1]:
            raise ValueError(f"a {kh}x{kw} kernel does not fit the {self.dims[0]} x {self.dims[1]} image")
        if not np.all(np.isfinite(h64)):
            raise ValueError("the taps of the kernel must be finite")
        self.h = h64
        self.offset = (kh // 2, kw // 2) if offset is None else (int(offset[0]), int(offset[1]))
        if not (0 <= self.offset[0] < kh and 0 <= self.offset[1] < kw):
            raise ValueError(f"offset {self.offset} outside the {kh}x{kw} kernel")
        self._mult = {}

    def gain(self):
        """G: the unnormalised DFT of the kernel wrapped about its origin, complex128 ``[H, W]``."""
        H, W = self.dims
        k = np.zeros(self.dims)
        kh, kw = self.h.shape
        ii = (np.arange(kh) - self.offset[0]) % H
        jj = (np.arange(kw) - self.offset[1]) % W
        np.add.at(k, (ii[:, None], jj[None, :]), self.h)
        return np.fft.fft2(k)

    def data(self, b):
        """F(observation) of a real observation ``b`` of the image's size."""
        a = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
        if np.iscomplexobj(a):
            raise ValueError("L2 with PeriodicConvolve2D: b is the real observation (its transform is taken here)")
        if a.size != self.dims[0] * self.dims[1]:
            raise ValueError(f"L2 with PeriodicConvolve2D: {a.size} observations for an image of shape {self.dims}")
        a = a.astype(np.float64).reshape(self.dims)
        if not np.all(np.isfinite(a)):
            raise ValueError("L2 with PeriodicConvolve2D: b must be finite")
        return np.fft.fft2(a, norm="ortho")

    def _multiplier(self, adjoint, dev):
        key = (bool(adjoint), dev)
        if key not in self._mult:
            G = self.gain()[:, : self.dims[1] // 2 + 1]
            if adjoint:
                G = np.conj(G)
            self._mult[key] = _dev.to_dev(np.stack([G.real, G.imag]), dev)
        return self._mult[key]

    def _apply(self, x, adjoint):
        import torch
        t, n_img, _ = self._batch(x, self.shape[1])
        out = torch.empty_like(t)
        m = self._multiplier(adjoint, t.device)
        _dev.run(t, "lmc_spectral_filter", _dev.ptr(t), _dev.ptr(out), n_img, self.dims[0], self.dims[1], _dev.ptr(m))
        return _dev.like_input(out.reshape(tuple(np.shape(x))), x)

    def matvec(self, x):
        return self._apply(x, False)

    def rmatvec(self, y):
        return self._apply(y, True)
