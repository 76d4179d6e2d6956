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
