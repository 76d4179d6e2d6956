"""Posterior summaries over the kept samples: the checked descriptors of a sampler's four optional accumulators (block moments, pixel histograms, chain-group
moments, covariance sketch), their stateless passes, and the arithmetic on accumulated sums.  Nothing here samples; ``algs.py`` re-exports every name."""
from __future__ import annotations

import numpy as np
import torch
from numpy.random import default_rng

from . import _capi, _dev


def mean_var_from_moments(s1, s2, count):
    """Posterior mean and pixel-wise variance from accumulated sums (any array type)."""
    mean = s1 / count
    var = s2 / count - mean * mean
    return mean, var


MOMENT_SCALES = (2, 4, 8, 16)


def _check_moment_scales(moment_scales, moments):
    """The tuple of block sizes a sampler is asked to keep second moments for (``None`` / empty = none); raises before any device call."""
    scales = tuple(int(v) for v in (moment_scales or ()))
    if scales and not moments:
        raise ValueError("moment_scales needs moments=True: the block moments are accumulated over the kept samples of the pixel moments")
    if len(set(scales)) != len(scales) or any(v not in MOMENT_SCALES for v in scales):
        raise ValueError(f"moment_scales must be distinct values out of {MOMENT_SCALES}, got {scales}")
    return scales


def block_mean_var(S1, S2, count, scale, dims):
    """Mean and variance of the block MEAN at one scale from the block-sum accumulators of :meth:`MYULASampler.block_moments`
    (torch tensors or numpy arrays ``[ceil(H/scale), ceil(W/scale)]``).  Every block is divided by its own pixel count, so the partial
    blocks at the bottom and right edges of an image whose sides are no multiple of ``scale`` need no special rule."""
    H, W = int(dims[0]), int(dims[1])
    s = int(scale)
    rows = np.minimum(s, H - s * np.arange(-(-H // s)))
    cols = np.minimum(s, W - s * np.arange(-(-W // s)))
    npix = np.outer(rows, cols).astype(np.float64)
    if isinstance(S1, torch.Tensor):
        npix = torch.as_tensor(npix, dtype=S1.dtype, device=S1.device)
    mean = S1 / (count * npix)
    var = S2 / (count * npix * npix) - mean * mean
    return mean, var


HIST_MAX_BINS = 62


def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _hist_arrays(bins, lo, hi, dims):
    """``(B, lo, scale)`` of a histogram of ``B`` bins over ``[lo, hi)`` per pixel: fp32 ``[H, W]`` numpy arrays, ``scale`` = bins per unit
    formed once as ``float32(B) / (float32(hi) - float32(lo))``.  Raises ``ValueError`` for what no histogram can be made of."""
    B = int(bins)
    if not 1 <= B <= HIST_MAX_BINS:
        raise ValueError(f"hist_bins must be 1 .. {HIST_MAX_BINS}, got {B}")
    shape = (int(dims[0]), int(dims[1]))
    try:
        lo32 = np.ascontiguousarray(np.broadcast_to(_host_array(lo).astype(np.float32), shape))
        hi32 = np.ascontiguousarray(np.broadcast_to(_host_array(hi).astype(np.float32), shape))
    except ValueError:
        raise ValueError(f"hist_range: lo and hi must be scalars or arrays of the image shape {shape}") from None
    if not (np.isfinite(lo32).all() and np.isfinite(hi32).all()):
        raise ValueError("hist_range: lo and hi must be finite at every pixel")
    if (hi32 <= lo32).any():
        raise ValueError("hist_range: hi must be above lo at every pixel (in fp32)")
    scale = np.float32(B) / (hi32 - lo32)
    if not np.isfinite(scale).all():
        raise ValueError("hist_range: hi - lo is too small for fp32 at some pixel")
    return B, lo32, scale.astype(np.float32)


def _check_histogram(hist_bins, hist_range, moments, dims):
    """``None`` or ``(B, lo, scale)`` of the histogram a sampler is asked to keep; raises before any device call."""
    if hist_bins is None and hist_range is None:
        return None
    if hist_bins is None or hist_range is None:
        raise ValueError("hist_bins and hist_range go together: the bins of a pixel histogram need their range (lo, hi)")
    if not moments:
        raise ValueError("hist_bins needs moments=True: the histogram is accumulated over the kept samples of the pixel moments")
    if not isinstance(hist_range, (tuple, list)) or len(hist_range) != 2:
        raise ValueError("hist_range must be (lo, hi), each a scalar or an [H, W] array")
    return _hist_arrays(hist_bins, hist_range[0], hist_range[1], dims)


def _hist_host(counts, lo, scale):
    c = _host_array(counts).astype(np.int64)
    if c.ndim != 3 or c.shape[0] < 3:
        raise ValueError("counts must be [B + 2, H, W]")
    lo64 = np.broadcast_to(_host_array(lo).astype(np.float64), c.shape[1:])
    sc64 = np.broadcast_to(_host_array(scale).astype(np.float64), c.shape[1:])
    return c, lo64, sc64


def hist_quantiles(counts, lo, scale, q):
    """Pixel-wise quantiles ``[len(q), H, W]`` (float64) from the counters ``[B + 2, H, W]`` of a pixel histogram (:meth:`MYULASampler.histogram`,
    :func:`pixel_histogram`) with its ``lo`` and ``scale`` (bins per unit).  Per pixel, with ``n`` the sum of the rows, ``r = q n``, ``cum`` the
    running sum over the rows and ``j`` the first row with ``cum_j >= r``: ``lo + (j - 1 + (r - cum_{j-1}) / counts_j) / scale``, i.e. linear inside
    the bin that holds the quantile.  ``j = 0`` gives ``-inf`` and ``j = B + 1`` gives ``+inf``: a quantile outside the chosen range is reported as
    infinite, not clamped -- the sign to widen the range.  By the same rule ``q = 0`` is ``-inf`` everywhere (row 0 already has ``cum_0 >= 0``): ask for a
    small positive ``q`` instead.  A pixel without samples gives NaN.  torch in, torch out (on the device of ``counts``);
    the arithmetic is on the host."""
    c, lo64, sc64 = _hist_host(counts, lo, scale)
    B = c.shape[0] - 2
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if qs.ndim != 1 or ((qs < 0) | (qs > 1)).any():
        raise ValueError("q must be probabilities in [0, 1]")
    cum = np.cumsum(c, axis=0)
    n = cum[-1]
    out = np.empty((len(qs),) + c.shape[1:], dtype=np.float64)
    for i, qq in enumerate(qs):
        r = qq * n.astype(np.float64)
        j = (cum < r[None]).sum(axis=0)                               # the first row with cum_j >= r
        jm = np.clip(j, 1, B)
        below = np.take_along_axis(cum, (jm - 1)[None], axis=0)[0]
        inbin = np.take_along_axis(c, jm[None], axis=0)[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = lo64 + (jm - 1 + (r - below) / inbin) / sc64
        v = np.where(j == 0, -np.inf, np.where(j == B + 1, np.inf, v))
        out[i] = np.where(n == 0, np.nan, v)
    return torch.from_numpy(out).to(counts.device) if isinstance(counts, torch.Tensor) else out


def hist_exceedance(counts, lo, scale, t):
    """Pixel-wise exceedance probability from the counters of a pixel histogram: the fraction of the samples in the rows from the first row
    whose lower edge ``lo + (j - 1) / scale`` is at or above ``t`` (a scalar or ``[H, W]``) upwards, the row above the range included.  The
    resolution is the bin width ``1 / scale``: it is P(x >= edge) for the first bin edge at or above ``t`` -- exact for ``t`` on an edge, and
    otherwise below P(x >= t) by at most the mass of the bin ``t`` lies in; for ``t`` below ``lo`` (``-inf`` included) the edge is ``lo`` itself, and
    ``t = +inf`` gives 0.  A NaN in ``t`` raises ``ValueError``.  ``[H, W]`` float64; torch in, torch out."""
    c, lo64, sc64 = _hist_host(counts, lo, scale)
    B = c.shape[0] - 2
    t64 = np.broadcast_to(_host_array(t).astype(np.float64), c.shape[1:])
    if np.isnan(t64).any():
        raise ValueError("hist_exceedance: t must not be NaN")
    first = np.clip(1 + np.ceil((t64 - lo64) * sc64), 1, B + 2).astype(np.int64)
    rows = np.arange(B + 2)[:, None, None]
    n = c.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(rows >= first[None], c, 0).sum(axis=0) / n.astype(np.float64)
    return torch.from_numpy(out).to(counts.device) if isinstance(counts, torch.Tensor) else out


def pixel_histogram(x, bins, lo, hi, out=None):
    """Pixel-wise histogram of the images ``x`` (``[C, H, W]``): counters ``[bins + 2, H, W]`` (``torch.int64`` on the device) over ``bins`` equal
    bins of ``[lo, hi)`` (scalars or ``[H, W]`` arrays), row 0 below the range and row ``bins + 1`` at or above it (NaN included).  Stateless
    (``lmc_pixel_histogram``); with ``out`` it ADDS into that tensor and returns it."""
    xt = _dev.to_dev(x)
    if xt.dim() != 3:
        raise ValueError("x must be [C, H, W]")
    Cn, H, W = (int(v) for v in xt.shape)
    B, lo32, sc32 = _hist_arrays(bins, lo, hi, (H, W))
    if out is None:
        out = torch.zeros((B + 2, H, W), dtype=torch.int64, device=xt.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.int64 and tuple(out.shape) == (B + 2, H, W) and out.is_contiguous()
              and out.device == xt.device):
        raise ValueError(f"out must be a contiguous torch.int64 tensor {(B + 2, H, W)} on {xt.device}")
    lo_d, sc_d = _dev.to_dev(lo32, xt.device), _dev.to_dev(sc32, xt.device)
    _dev.run(xt, "lmc_pixel_histogram", _dev.ptr(xt), Cn, H, W, B, _dev.ptr(lo_d), _dev.ptr(sc_d), _dev.ptr(out))
    torch.cuda.current_stream(xt.device).synchronize()          # lo_d / sc_d live until the launch is done
    return out


def _hist_summaries(smp, quantiles):
    """``(counts, lo, scale, {q: tensor [H, W]})`` of a sampler's histogram; Nones and an empty dict without one."""
    if smp.hist_bins is None:
        return None, None, None, {}
    counts, _ = smp.histogram()
    qs = tuple(float(v) for v in (quantiles or ()))
    vals = hist_quantiles(counts, smp.hist_lo, smp.hist_scale, qs) if qs else ()
    return counts, smp.hist_lo, smp.hist_scale, {qv: vals[i] for i, qv in enumerate(qs)}


MAX_CHAIN_GROUPS = _capi.MAX_CHAIN_GROUPS


def _check_chain_groups(chain_groups, moments, n_chains=None):
    """``None`` or the number of chain groups a sampler is asked to keep moments for; raises before any device call.  ``n_chains``: the entry
    points refuse more groups than chains (an empty group has no mean); a sampler accepts them, as the library does."""
    if chain_groups is None:
        return None
    G = int(chain_groups)
    if not 2 <= G <= MAX_CHAIN_GROUPS:
        raise ValueError(f"chain_groups must be 2 .. {MAX_CHAIN_GROUPS}, got {G}")
    if not moments:
        raise ValueError("chain_groups needs moments=True: the group moments are accumulated over the kept samples of the pixel moments")
    if n_chains is not None and G > int(n_chains):
        raise ValueError(f"chain_groups = {G} exceeds n_chains = {int(n_chains)}: every group needs a chain")
    return G


def group_moments(x, n_groups, chain_offset=0, out=None):
    """Chain-group moments of the images ``x`` (``[C, H, W]``): ``(S1, S2)``, float64 ``[n_groups, H, W]`` on the device, the sums of x and of
    x^2 over the chains of every group -- chain ``c`` belongs to group ``(chain_offset + c) % n_groups``.  Stateless (``lmc_group_moments``);
    with ``out=(S1, S2)`` it ADDS into those tensors and returns them.  No atomics: equal calls give equal bits."""
    xt = _dev.to_dev(x)
    if xt.dim() != 3:
        raise ValueError("x must be [C, H, W]")
    G = int(n_groups)
    if not 2 <= G <= MAX_CHAIN_GROUPS:
        raise ValueError(f"n_groups must be 2 .. {MAX_CHAIN_GROUPS}, got {G}")
    if int(chain_offset) < 0:
        raise ValueError("chain_offset must be >= 0")
    Cn, H, W = (int(v) for v in xt.shape)
    if out is None:
        out = (torch.zeros((G, H, W), dtype=torch.float64, device=xt.device), torch.zeros((G, H, W), dtype=torch.float64, device=xt.device))
    elif not (isinstance(out, (tuple, list)) and len(out) == 2 and all(
            isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == (G, H, W) and t.is_contiguous() and t.device == xt.device
            for t in out)):
        raise ValueError(f"out must be two contiguous torch.float64 tensors {(G, H, W)} on {xt.device}")
    if out[0].data_ptr() == out[1].data_ptr():
        raise ValueError("out must be two DISTINCT tensors: the sums of x and of x^2 do not share an array")
    _dev.run(xt, "lmc_group_moments", _dev.ptr(xt), Cn, int(chain_offset), H, W, G, _dev.ptr(out[0]), _dev.ptr(out[1]))
    torch.cuda.current_stream(xt.device).synchronize()          # xt may be a temporary
    return out[0], out[1]


class GroupMCSE:
    """What :func:`mcse_from_group_moments` returns, per pixel in float64: ``mean``, ``var`` (pooled over all groups), ``mcse_mean`` and
    ``mcse_var`` (the Monte-Carlo standard errors of the two) and ``ess`` (the effective sample size of the mean)."""

    def __init__(self, mean, var, mcse_mean, mcse_var, ess):
        self.mean, self.var, self.mcse_mean, self.mcse_var, self.ess = mean, var, mcse_mean, mcse_var, ess


def mcse_from_group_moments(S1, S2, counts):
    """Pixel-wise Monte-Carlo error of the posterior mean and variance from chain-group moments (:meth:`MYULASampler.group_moments`,
    :func:`group_moments`): ``S1``, ``S2`` ``[G, H, W]`` = the sums of x and x^2 per group, ``counts`` ``[G]`` = the samples per group.  With
    ``N = sum n``, ``m_g = S1_g / n_g``, ``v_g = S2_g / n_g - m_g^2``, ``m = sum S1_g / N`` and ``v = sum S2_g / N - m^2``:

    * ``mcse_mean = sqrt(s / N)``, ``s = sum_g n_g (m_g - m)^2 / (G - 1)``;
    * ``mcse_var = sqrt(sv / N)``, ``sv = sum_g n_g (v_g - vbar)^2 / (G - 1)``, ``vbar = sum n_g v_g / N``;
    * ``ess = N v / s``, ``+inf`` where ``s = 0`` (not a clamp).

    For equal counts this is the textbook standard error of G independent replicate means: the scatter of the group means carries the
    autocorrelation of the chains, with no lags and no stored iterate; the weights keep it unbiased when the chain count is no multiple of G.
    The relative precision of ``s`` is ``sqrt(2 / (G - 1))`` -- about 25 % at G = 32 and 18 % at G = 64 (which is why the library allows up to 64
    groups, not 8): read single pixels of these maps with that in mind, medians and smoothed maps are far tighter.  numpy in, numpy out; torch in,
    torch out (on the device of ``S1``); float64, the arithmetic is on the host.  ``ValueError`` for fewer than 2 groups or a group without
    samples."""
    a, b = _host_array(S1).astype(np.float64), _host_array(S2).astype(np.float64)
    n = _host_array(counts).astype(np.float64).reshape(-1)
    if a.ndim < 1 or a.shape != b.shape or a.shape[0] != n.size:
        raise ValueError("S1 and S2 must be [G, ...] of one shape and counts [G]")
    G = n.size
    if G < 2:
        raise ValueError("the Monte-Carlo error needs at least 2 chain groups")
    if (n <= 0).any():
        raise ValueError("every chain group needs samples: a count of 0 has no group mean (fewer groups than chains avoid it)")
    ng = n.reshape((G,) + (1,) * (a.ndim - 1))
    N = n.sum()
    mg = a / ng
    vg = b / ng - mg * mg
    mean = a.sum(axis=0) / N
    var = b.sum(axis=0) / N - mean * mean
    s = (ng * (mg - mean) ** 2).sum(axis=0) / (G - 1)
    vbar = (ng * vg).sum(axis=0) / N
    sv = (ng * (vg - vbar) ** 2).sum(axis=0) / (G - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(s == 0, np.inf, N * var / s)
    parts = (mean, var, np.sqrt(s / N), np.sqrt(sv / N), ess)
    if isinstance(S1, torch.Tensor):
        parts = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(S1.device) for v in parts)
    return GroupMCSE(*parts)


def _group_summaries(smp):
    """``(mcse_mean, mcse_var, ess, counts)`` of a sampler's chain-group moments; None without them."""
    if smp.chain_groups is None:
        return None
    S1, S2, counts = smp.group_moments()
    r = mcse_from_group_moments(S1, S2, counts)
    return r.mcse_mean, r.mcse_var, r.ess, counts


MAX_COV_PROBES = _capi.MAX_COV_PROBES


def _check_cov_sketch(cov_probes, cov_center, moments, dims):
    """``None`` or ``(k, probes fp32 [k, H*W], centre fp32 [H*W] or None)`` (host arrays) of the covariance sketch a sampler is asked to keep;
    raises ``ValueError`` before any device call."""
    if cov_probes is None:
        if cov_center is not None:
            raise ValueError("cov_center without cov_probes: the centre belongs to the covariance sketch")
        return None
    H, W = int(dims[0]), int(dims[1])
    n = H * W
    P = np.asarray(_host_array(cov_probes), dtype=np.float32)
    if not ((P.ndim == 3 and P.shape[1:] == (H, W)) or (P.ndim == 2 and P.shape[1] == n)):
        raise ValueError(f"cov_probes must be [k, {H}, {W}] or [k, {n}], got {tuple(P.shape)}")
    k = int(P.shape[0])
    if not 1 <= k <= MAX_COV_PROBES:
        raise ValueError(f"cov_probes: the number of probes must be 1 .. {MAX_COV_PROBES}, got {k}")
    P = np.ascontiguousarray(P.reshape(k, n))
    if not np.isfinite(P).all():
        raise ValueError("cov_probes must be finite")
    m = None
    if cov_center is not None:
        m = np.asarray(_host_array(cov_center), dtype=np.float32)
        if m.size != n or m.shape not in ((H, W), (n,)):
            raise ValueError(f"cov_center must be [{H}, {W}] or [{n}], got {tuple(m.shape)}")
        m = np.ascontiguousarray(m.reshape(n))
        if not np.isfinite(m).all():
            raise ValueError("cov_center must be finite")
    if not moments:
        raise ValueError("cov_probes needs moments=True: the covariance sketch is accumulated over the kept samples of the pixel moments")
    return k, P, m


def cov_sketch(x, probes, center=None, out=None):
    """Covariance sketch of the images ``x`` (``[C, H, W]``) against the probe images ``probes`` (``[k, H, W]`` or ``[k, H*W]``, 1 <= k <= 32) about
    ``center`` (``[H, W]`` or flat, ``None`` = 0): ``(Y, s, Q)``, float64 on the device, ``Y[k, H, W] = sum_c t_c d_c``, ``s[k] = sum_c t_c``,
    ``Q[k, k] = sum_c t_c t_c^T`` with ``d_c = x_c - center`` (fp32) and ``t_c = probes . d_c``.  Stateless (``lmc_cov_sketch``); with
    ``out=(Y, s, Q)`` it ADDS into those tensors and returns them.  No atomics: equal calls give equal bits.  :func:`cov_from_sketch` turns the
    sums into covariances."""
    if not (hasattr(x, "shape") and len(x.shape) == 3):
        raise ValueError("x must be [C, H, W]")
    Cn, H, W = (int(v) for v in x.shape)
    k, P, m = _check_cov_sketch(probes, center, True, (H, W))
    xt = _dev.to_dev(x)
    P_d = _dev.to_dev(P, xt.device)
    m_d = None if m is None else _dev.to_dev(m, xt.device)
    shapes = ((k, H, W), (k,), (k, k))
    if out is None:
        out = tuple(torch.zeros(s, dtype=torch.float64, device=xt.device) for s in shapes)
    elif not (isinstance(out, (tuple, list)) and len(out) == 3 and all(
            isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == s and t.is_contiguous() and t.device == xt.device
            for t, s in zip(out, shapes))):
        raise ValueError(f"out must be three contiguous torch.float64 tensors {shapes} on {xt.device}")
    nbytes = int(_dev.lib().lmc_cov_sketch_workspace_bytes(Cn, H, W, k))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=xt.device)
    _dev.run(xt, "lmc_cov_sketch", _dev.ptr(xt), Cn, H, W, k, _dev.ptr(P_d), _dev.ptr(m_d), _dev.ptr(out[0]), _dev.ptr(out[1]), _dev.ptr(out[2]),
             _dev.ptr(ws))
    torch.cuda.current_stream(xt.device).synchronize()          # xt, the probes and the workspace may be temporaries
    return out[0], out[1], out[2]


class CovSketch:
    """What :func:`cov_from_sketch` returns, float64 numpy arrays: ``cov_xt`` ``[k, H, W]`` (the covariance of every pixel with projection j, row j
    of ``P Sigma``), ``cov_tt`` ``[k, k]`` (``P Sigma P^T``), ``t_mean`` ``[k]`` (the mean projections) and ``n`` (the samples)."""

    def __init__(self, cov_xt, cov_tt, t_mean, n):
        self.cov_xt, self.cov_tt, self.t_mean, self.n = cov_xt, cov_tt, t_mean, n

    def corr(self, var):
        """Correlation maps ``[k, H, W]``: ``cov_xt[j] / sqrt(var * cov_tt[j, j])`` with the pixel variance ``var`` (``[H, W]``).  NaN where a
        variance (of the pixel or of the projection) is 0 or negative -- not a clamp."""
        v = _host_array(var).astype(np.float64).reshape(self.cov_xt.shape[1:])
        den = v[None] * np.diag(self.cov_tt).reshape((-1,) + (1,) * v.ndim)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, self.cov_xt / np.sqrt(den), np.nan)

    def modes(self, rank, rcond=1e-10):
        """``(eigenvalues [rank], eigen-images [rank, H, W])`` of the Nystrom approximation ``Sigma ~ cov_xt^T cov_tt^+ cov_xt``, largest first.
        ``cov_tt`` is symmetrised and decomposed (``eigh``), eigenvalues ``<= rcond * max`` are dropped, ``B = cov_xt^T V w^{-1/2}`` of the kept
        pairs has ``Sigma ~ B B^T``; its singular values squared and left vectors are returned.  Exact when the rank of the sample covariance is at
        most the number of probes (Gaussian probes, :func:`random_probes`); otherwise the eigenvalues are UNDERESTIMATED, as Nystrom
        approximations of a positive semi-definite matrix always are -- read them as lower bounds.  ``ValueError`` if ``rank`` exceeds the number
        of eigenvalues kept."""
        k = self.cov_tt.shape[0]
        w, V = np.linalg.eigh(0.5 * (self.cov_tt + self.cov_tt.T))
        keep = w > float(rcond) * max(float(w.max()), 0.0)
        r = int(rank)
        if r < 1 or r > int(keep.sum()):
            raise ValueError(f"rank = {r}: the sketch keeps {int(keep.sum())} of {k} directions (rcond = {rcond})")
        B = self.cov_xt.reshape(k, -1).T @ (V[:, keep] / np.sqrt(w[keep]))
        U, sv, _ = np.linalg.svd(B, full_matrices=False)
        return sv[:r] ** 2, np.ascontiguousarray(U[:, :r].T).reshape((r,) + self.cov_xt.shape[1:])


def cov_from_sketch(Y, s, Q, n, s1, center=None):
    """Covariances from the sums of a covariance sketch (:meth:`MYULASampler.cov_sketch`, :func:`cov_sketch`) and the pixel sums ``s1`` of the same
    ``n`` samples: with ``dbar = s1 / n - center`` and ``tbar = s / n``, a :class:`CovSketch` of ``cov_xt = Y / n - tbar dbar`` -- exactly
    ``P Sigma``, ``Sigma`` the sample covariance (``np.cov(bias=True)``) of the samples as flat images -- and ``cov_tt = Q / n - tbar tbar^T``
    -- exactly ``P Sigma P^T``.  ``center`` must be the one the sums were formed with.  float64 on the host.  Without a centre ``cov_xt`` is a
    difference of terms of size mean^2 and loses digits: form the sums about a pilot-run mean."""
    Yh, sh, Qh = (_host_array(v).astype(np.float64) for v in (Y, s, Q))
    n = int(n)
    if n < 1:
        raise ValueError("the covariance sketch holds no samples")
    if Yh.ndim < 2 or sh.shape != (Yh.shape[0],) or Qh.shape != (Yh.shape[0], Yh.shape[0]):
        raise ValueError("Y must be [k, H, W] (or [k, H*W]), s [k] and Q [k, k]")
    k = Yh.shape[0]
    dbar = _host_array(s1).astype(np.float64).reshape(Yh.shape[1:]) / n
    if center is not None:
        dbar = dbar - _host_array(center).astype(np.float32).astype(np.float64).reshape(Yh.shape[1:])
    tbar = sh / n
    cov_xt = Yh / n - tbar.reshape((k,) + (1,) * (Yh.ndim - 1)) * dbar[None]
    return CovSketch(cov_xt, Qh / n - np.outer(tbar, tbar), tbar, n)


def random_probes(k, dims, seed=0):
    """``k`` Gaussian random probe images ``[k, H, W]`` (fp32 numpy) from ``numpy.random.default_rng(seed)``: the probes of the Nystrom sketch
    (:meth:`CovSketch.modes`).  Every rank of a sharded job must use the same ``seed``."""
    k = int(k)
    if not 1 <= k <= MAX_COV_PROBES:
        raise ValueError(f"k must be 1 .. {MAX_COV_PROBES}, got {k}")
    return default_rng(seed).standard_normal((k, int(dims[0]), int(dims[1]))).astype(np.float32)


def _cov_summary(smp, s1):
    """The :class:`CovSketch` of a sampler's covariance sketch and pixel sums ``s1``; None without one (or without samples)."""
    if smp.cov_k is None:
        return None
    Y, s, Q, n = smp.cov_sketch()
    return cov_from_sketch(Y, s, Q, n, s1, smp.cov_center) if n else None


def _scale_summaries(smp):
    """``({scale: mean}, {scale: std})`` of the block means of every scale the sampler keeps."""
    means, stds = {}, {}
    for sc in smp.moment_scales:
        S1, S2, cnt = smp.block_moments(sc)
        m, v = block_mean_var(S1, S2, max(cnt, 1), sc, smp.dims)
        means[sc], stds[sc] = m, v.clamp_min(0).sqrt()
    return means, stds


ACCUMULATOR_KEYWORDS = ("moment_scales", "hist_bins", "hist_range", "chain_groups", "cov_probes", "cov_center")


def _check_accumulators(kw, moments, dims, n_chains=None):
    """``(scales, hist, groups, cov)`` as the four ``_check_*`` return them, from a mapping with any of ``ACCUMULATOR_KEYWORDS`` (a missing one is
    ``None``); raises before any device call.  One order of checks for every sampler, so the same error wins when several arguments are wrong."""
    return (_check_moment_scales(kw.get("moment_scales"), moments),
            _check_histogram(kw.get("hist_bins"), kw.get("hist_range"), moments, dims),
            _check_chain_groups(kw.get("chain_groups"), moments, n_chains),
            _check_cov_sketch(kw.get("cov_probes"), kw.get("cov_center"), moments, dims))
