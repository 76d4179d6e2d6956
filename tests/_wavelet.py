"""float64 checker of the Daubechies wavelet-l1 prior (LMC_PRIOR_WAVELET_L1; include/lmc_atomi.h and the issue text are the definition).  numpy only.

* `scaling_filter(p)`: the extremal-phase filter by spectral factorisation -- P(y) = sum_{k<p} C(p-1+k, k) y^k with y = (2 - z - 1/z)/4, of every
  root pair {z, 1/z} the root inside the unit circle, times (1 + z)^p, normalised to sum sqrt(2).  `wavelet_filter`: g[k] = (-1)^k h[2p-1-k].
* `analysis_matrix(p, n)`: one level on a periodic signal of even length n >= 2p as an n x n matrix, lo rows first:
  lo[m] = sum_k h[k] a[(2m+k) mod n], hi[m] = sum_k g[k] a[(2m+k) mod n].
* `dwt2`, `idwt2`, `prox`, `value`: the 2-D transform in Mallat layout (rows first, then columns; deeper levels on the top-left quarter), by those
  matrices, in the dtype of the input ("every routine computes in the dtype of its input").
* `dwt2_taps`, `idwt2_taps`, `prox_taps`: the same in a second form, a direct tap loop over strided views, also dtype-generic: the float32 replays of
  the two forms associate their sums differently, and the larger of their deviations from float64 is the e32 of tests/_pixel.bound_of.
"""
import functools
from math import comb

import numpy as np

MAX_LEVELS = 8


@functools.lru_cache(maxsize=None)
def _scaling(p):
    if p < 1:
        raise ValueError("p >= 1")
    zs = []
    if p > 1:
        coef = [float(comb(p - 1 + k, k)) for k in range(p)]          # ascending powers of y
        for y in np.roots(coef[::-1]):
            b = 2.0 - 4.0 * y                                         # z^2 - b z + 1 = 0
            d = np.sqrt(b * b - 4.0 + 0j)
            big = (b + d) / 2 if abs(b + d) >= abs(b - d) else (b - d) / 2
            zs.append(1.0 / big)                                      # the root inside the unit circle, without cancellation
    h = np.array([1.0 + 0j])
    for z in zs:
        h = np.convolve(h, [1.0, -z])
    for _ in range(p):
        h = np.convolve(h, [1.0, 1.0])
    assert np.max(np.abs(h.imag)) < 1e-12 * np.max(np.abs(h.real))
    h = h.real
    h = h * (np.sqrt(2.0) / h.sum())
    h.setflags(write=False)
    return h


def scaling_filter(p):
    return _scaling(int(p))


def wavelet_filter(p):
    h = scaling_filter(p)
    n = h.size
    return np.array([(-1.0) ** k * h[n - 1 - k] for k in range(n)])


def check_shape(shape, p, levels):
    H, W = shape
    if not 1 <= p <= 4:
        raise ValueError("p in 1..4")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels in 1..8")
    if H % (1 << levels) or W % (1 << levels):
        raise ValueError("sides must be multiples of 2^levels")
    if (min(H, W) >> (levels - 1)) < 2 * p:
        raise ValueError("coarsest input shorter than the filter")


def legal(shape, p, levels):
    try:
        check_shape(shape, p, levels)
    except ValueError:
        return False
    return True


@functools.lru_cache(maxsize=None)
def _analysis(p, n):
    h, g = scaling_filter(p), wavelet_filter(p)
    if n % 2 or n < 2 * p:
        raise ValueError("even n >= 2p")
    A = np.zeros((n, n))
    for m in range(n // 2):
        for k in range(2 * p):
            A[m, (2 * m + k) % n] += h[k]
            A[n // 2 + m, (2 * m + k) % n] += g[k]
    A.setflags(write=False)
    return A


def analysis_matrix(p, n, dtype=np.float64):
    return _analysis(int(p), int(n)).astype(dtype)


# ---- the matrix form -------------------------------------------------------------------------------------------------------------------------
def dwt2(x, p, levels):
    x = np.asarray(x)
    c = x.copy()
    H, W = x.shape[-2:]
    check_shape((H, W), p, levels)
    for j in range(levels):
        h, w = H >> j, W >> j
        blk = c[..., :h, :w]
        blk = blk @ analysis_matrix(p, w, x.dtype).T                  # along the rows
        blk = analysis_matrix(p, h, x.dtype) @ blk                    # along the columns
        c[..., :h, :w] = blk
    assert c.dtype == x.dtype
    return c


def idwt2(c, p, levels):
    c = np.asarray(c)
    x = c.copy()
    H, W = c.shape[-2:]
    check_shape((H, W), p, levels)
    for j in range(levels - 1, -1, -1):
        h, w = H >> j, W >> j
        blk = x[..., :h, :w]
        blk = analysis_matrix(p, h, c.dtype).T @ blk
        blk = blk @ analysis_matrix(p, w, c.dtype)
        x[..., :h, :w] = blk
    assert x.dtype == c.dtype
    return x


def detail_mask(shape, levels):
    m = np.ones(shape, dtype=bool)
    m[:shape[0] >> levels, :shape[1] >> levels] = False
    return m


def soft(c, t):
    return np.sign(c) * np.maximum(np.abs(c) - c.dtype.type(t), c.dtype.type(0))


def _threshold(c, levels, thr):
    m = detail_mask(c.shape[-2:], levels)
    out = c.copy()
    out[..., m] = soft(c[..., m], thr)
    return out


def prox(x, p, levels, thr):
    """W^T S(W x): the details soft-thresholded by thr, the approximation untouched."""
    x = np.asarray(x)
    return idwt2(_threshold(dwt2(x, p, levels), levels, thr), p, levels)


def value(x, p, levels, sigma=1.0):
    """sigma * sum |detail coefficients|, one number per image (float64 whatever the dtype of x)."""
    c = dwt2(np.asarray(x), p, levels)
    m = detail_mask(c.shape[-2:], levels)
    return sigma * np.abs(c[..., m].astype(np.float64)).sum(axis=-1)


# ---- the tap-loop form -----------------------------------------------------------------------------------------------------------------------
def _analyse_last(a, p):
    """One level along the last axis: (lo, hi), sums in tap order, in the dtype of a."""
    h, g = scaling_filter(p).astype(a.dtype), wavelet_filter(p).astype(a.dtype)
    n = a.shape[-1]
    lo = np.zeros(a.shape[:-1] + (n // 2,), dtype=a.dtype)
    hi = np.zeros_like(lo)
    for k in range(2 * p):
        s = np.roll(a, -k, axis=-1)[..., ::2]
        lo = lo + h[k] * s
        hi = hi + g[k] * s
    return lo, hi


def _synthesise_last(lo, hi, p):
    """The adjoint: x[2j+e] = sum_q h[2q+e] lo[j-q] + g[2q+e] hi[j-q] (indices mod n/2)."""
    h, g = scaling_filter(p).astype(lo.dtype), wavelet_filter(p).astype(lo.dtype)
    x = np.zeros(lo.shape[:-1] + (2 * lo.shape[-1],), dtype=lo.dtype)
    for e in (0, 1):
        acc = np.zeros_like(lo)
        for q in range(p):
            acc = acc + h[2 * q + e] * np.roll(lo, q, axis=-1) + g[2 * q + e] * np.roll(hi, q, axis=-1)
        x[..., e::2] = acc
    return x


def dwt2_taps(x, p, levels):
    x = np.asarray(x)
    c = x.copy()
    H, W = x.shape[-2:]
    check_shape((H, W), p, levels)
    for j in range(levels):
        h, w = H >> j, W >> j
        lo, hi = _analyse_last(c[..., :h, :w], p)
        rows = np.concatenate([lo, hi], axis=-1)
        lo, hi = _analyse_last(np.swapaxes(rows, -1, -2), p)
        c[..., :h, :w] = np.swapaxes(np.concatenate([lo, hi], axis=-1), -1, -2)
    assert c.dtype == x.dtype
    return c


def idwt2_taps(c, p, levels):
    c = np.asarray(c)
    x = c.copy()
    H, W = c.shape[-2:]
    check_shape((H, W), p, levels)
    for j in range(levels - 1, -1, -1):
        h, w = H >> j, W >> j
        t = np.swapaxes(x[..., :h, :w], -1, -2)
        t = np.swapaxes(_synthesise_last(t[..., :h // 2], t[..., h // 2:], p), -1, -2)
        x[..., :h, :w] = _synthesise_last(t[..., :w // 2], t[..., w // 2:], p)
    assert x.dtype == c.dtype
    return x


def prox_taps(x, p, levels, thr):
    x = np.asarray(x)
    return idwt2_taps(_threshold(dwt2_taps(x, p, levels), levels, thr), p, levels)


def value_taps(x, p, levels, sigma=1.0):
    c = dwt2_taps(np.asarray(x), p, levels)
    m = detail_mask(c.shape[-2:], levels)
    return sigma * np.abs(c[..., m].astype(np.float64)).sum(axis=-1)


def replays(fn64, fn_a, fn_b, x32):
    """(ref64, the float32 replay that deviates most from it): fn64 on float64(x32), fn_a and fn_b on x32 itself."""
    ref64 = fn64(x32.astype(np.float64))
    ra, rb = fn_a(x32), fn_b(x32)
    assert ra.dtype == np.float32 and rb.dtype == np.float32
    ea = np.max(np.abs(ra.astype(np.float64) - ref64))
    eb = np.max(np.abs(rb.astype(np.float64) - ref64))
    return ref64, (ra if ea >= eb else rb)
