"""Yardsticks of the covariance sketch (include/lmc_atomi.h, lmc_sampler_set_cov_sketch), numpy only.

``sketch_ref``: the definition in float64 -- d = fp32(x - m) widened, t = P d, Y += t d, s += t, Q += t t^T.

``sketch_fp32``: the arithmetic contract restated with the loosest arithmetic it allows -- fp32 products added one by one in fp32 (two
roundings per term, where an fmaf chain has one) over runs of 2048 pixels for t, the run sums combined in float64 in ascending order; t rounded to
fp32 for the Y update, fp32 products added one by one in fp32 over runs of 1024 chains, the run sums added in float64; s and Q in float64 from the
float64 t.  Its distance from ``sketch_ref`` is what rounding of this kind costs on the data at hand: the yardstick of the device's rounding.
"""
import numpy as np

PIXEL_RUN = 2048
CHAIN_RUN = 1024


def centred(x, m):
    """d[C, N] fp32: one fp32 subtraction per element (m None = 0)"""
    x = np.asarray(x, dtype=np.float32).reshape(x.shape[0], -1)
    return x if m is None else (x - np.asarray(m, dtype=np.float32).reshape(1, -1)).astype(np.float32)


def sketch_ref(x, P, m=None):
    """(Y [k, N], s [k], Q [k, k]) float64 of x [C, ...], P [k, ...], m [...] by the definition"""
    d = centred(x, m).astype(np.float64)
    P64 = np.asarray(P, dtype=np.float64).reshape(len(P), -1)
    t = d @ P64.T                       # [C, k]
    return t.T @ d, t.sum(axis=0), t.T @ t


def _seq_sum_fp32(terms, axis):
    """sum of fp32 terms along ``axis``, added one by one in fp32 in ascending order (cumsum is sequential)"""
    return np.take(np.cumsum(terms, axis=axis, dtype=np.float32), -1, axis=axis)


def projections_fp32(d, P32):
    """t [C, k] float64: fp32 runs of PIXEL_RUN pixels, combined in float64 in ascending run order"""
    C, N = d.shape
    t = np.zeros((C, P32.shape[0]), dtype=np.float64)
    for a in range(0, N, PIXEL_RUN):
        prod = (d[:, None, a:a + PIXEL_RUN] * P32[None, :, a:a + PIXEL_RUN]).astype(np.float32)      # [C, k, run]
        t += _seq_sum_fp32(prod, 2).astype(np.float64)
    return t


def sketch_fp32(x, P, m=None):
    d = centred(x, m)
    P32 = np.asarray(P, dtype=np.float32).reshape(len(P), -1)
    t = projections_fp32(d, P32)
    tf = t.astype(np.float32)
    Y = np.zeros((P32.shape[0], d.shape[1]), dtype=np.float64)
    for a in range(0, d.shape[0], CHAIN_RUN):
        prod = (tf[a:a + CHAIN_RUN, :, None] * d[a:a + CHAIN_RUN, None, :]).astype(np.float32)       # [run, k, N]
        Y += _seq_sum_fp32(prod, 0).astype(np.float64)
    return Y, t.sum(axis=0), t.T @ t


def max_abs_errors(got, ref):
    return tuple(float(np.max(np.abs(np.asarray(g, dtype=np.float64).reshape(r.shape) - r))) for g, r in zip(got, ref))
