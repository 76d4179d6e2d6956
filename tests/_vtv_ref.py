"""The vectorial TV prior (LMC_PRIOR_VTV; include/lmc_atomi.h holds the definition) restated in numpy, dtype-generic ("every routine computes in the dtype
of its input"), with the case list and the cached references the CPU and GPU tests share.  numpy only.

    VTV(x) = sum_pixels sqrt(sum_ch (d_r x_ch)^2 + (d_c x_ch)^2)        channels on axis -3

`vtv_prox` is the loop of `oracle.lmc_oracle.tv_prox_fgp` with ONE projection weight per pixel over all channels; with one channel it is that function bit
for bit (tests/test_vtv_reference.py).  `form="rsqrt"` is the same loop in the arithmetic form of the kernel -- the weight as a reciprocal square root
that multiplies, where the definition divides by the root: the second float32 replay the bound of tests/_pixel.py asks for."""
import functools

import numpy as np

from oracle import lmc_oracle as O
import _pixel as PX

SHAPES = [(4, 4), (5, 7), (16, 24), (33, 70), (64, 136), (97, 261)]
CHANNELS = [1, 2, 3, 4]
PROX_PARAMS = [0.75, 2.5, 40.0]
ITERS = [1, 10, 23, 64]
N_IMAGES = 2


def _project(r, s, form, planted=None):
    """(p', q') of the dual step (r, s): the division by w = max(1, sqrt(sum_ch r^2 + s^2)).  `planted`: one of the faults the bound has to reject."""
    one = r.dtype.type(1)
    n2 = r * r + s * s
    if planted == "independent":            # channels projected independently
        tot = n2
    elif planted == "drop_last":            # the last channel left out of the norm
        tot = np.sum(n2[..., :-1, :, :], axis=-3, keepdims=True)
    elif planted == "max":                  # max over channels instead of the sum
        tot = np.max(n2, axis=-3, keepdims=True)
    elif planted == "columns_uncoupled":    # the row differences coupled, the column differences not
        tot = np.sum(r * r, axis=-3, keepdims=True) + s * s
    else:
        assert planted is None, planted
        tot = np.sum(n2, axis=-3, keepdims=True)
    if form == "rsqrt":
        inv = one / np.sqrt(np.maximum(tot, one))
        return r * inv, s * inv
    w = np.maximum(one, np.sqrt(tot))
    return r / w, s / w


def vtv_prox(x, gamma, niter, step=0.125, bounds=None, betas=None, form="div", planted=None, return_dual=False):
    """prox of gamma * VTV at x[..., nch, H, W]: `niter` dual iterations from the zero dual; `bounds=(lo, hi)`: every primal iterate clipped."""
    x = np.asarray(x)
    assert x.ndim >= 3
    dt = x.dtype
    gamma = dt.type(gamma)
    c = dt.type(step) / gamma
    betas = np.asarray(O.fgp_betas(niter) if betas is None else betas, dtype=dt)
    clip = (lambda v: v) if bounds is None else (lambda v: np.clip(v, dt.type(bounds[0]), dt.type(bounds[1])))
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    for k in range(niter):
        sol = clip(x - gamma * O.div2d(rr, ss))
        dr, dc = O.grad2d(sol)
        r = rr - c * dr
        s = ss - c * dc
        pn, qn = _project(r, s, form, planted)
        if return_dual and k == niter - 1:
            raw = (r, s)
        rr = pn + betas[k] * (pn - p)
        ss = qn + betas[k] * (qn - q)
        p, q = pn, qn
    out = clip(x - gamma * O.div2d(rr, ss))
    assert out.dtype == dt
    return (out, raw) if return_dual else out


def vtv_value(x):
    """VTV of x[..., nch, H, W], one value per multi-channel image."""
    dr, dc = O.grad2d(np.asarray(x))
    return np.sum(np.sqrt(np.sum(dr * dr + dc * dc, axis=-3)), axis=(-2, -1))


def data_grad(x, y, h, offset, mask, sigma_f):
    """sigma_f Op^T (Op x - y) per channel of x[nch, C, H, W]; y [nch, H, W] and mask ([H, W] or [nch, H, W]) broadcast over the chains."""
    dt = x.dtype
    if y is None:
        return np.zeros_like(x)
    yb = np.asarray(y, dtype=dt)[:, None]
    if mask is not None:
        m = np.asarray(mask, dtype=dt)
        m = m[:, None] if m.ndim == 3 else m
        return dt.type(sigma_f) * (m * (m * x - yb))
    if h is not None:
        hh = np.asarray(h, dtype=dt)
        return dt.type(sigma_f) * O.blur_adjoint(O.blur(x, hh, offset) - yb, hh, offset)
    return dt.type(sigma_f) * (x - yb)


def myula_step(x, y, h, offset, mask, sigma_f, tau, gamma, t_sigma, niter, xi, bounds=None, form="div"):
    """a x - tau grad f + b prox + sqrt(2 tau) xi on x[nch, C, H, W] (the state layout of the sampler), a = 1 - tau / gamma, b = tau / gamma."""
    x = np.asarray(x)
    dt = x.dtype
    g = data_grad(x, y, h, offset, mask, sigma_f)
    px = np.moveaxis(vtv_prox(np.moveaxis(x, 0, -3), t_sigma, niter, bounds=bounds, form=form), -3, 0) if t_sigma > 0 else x
    out = dt.type(1 - tau / gamma) * x - dt.type(tau) * g + dt.type(tau / gamma) * px + dt.type(np.sqrt(2 * tau)) * np.asarray(xi, dtype=dt)
    assert out.dtype == dt
    return out


def data_value(x, y, h, offset, mask, sigma_f):
    """f[c] = sum_ch sigma_f / 2 ||Op x_ch,c - y_ch||^2 of x[nch, C, H, W] in float64."""
    x = np.asarray(x, dtype=np.float64)
    if y is None:
        return np.zeros(x.shape[1])
    yb = np.asarray(y, dtype=np.float64)[:, None]
    if mask is not None:
        m = np.asarray(mask, dtype=np.float64)
        u = (m[:, None] if m.ndim == 3 else m) * x
    elif h is not None:
        u = O.blur(x, np.asarray(h, dtype=np.float64), offset)
    else:
        u = x
    return 0.5 * sigma_f * np.sum((u - yb) ** 2, axis=(0, 2, 3))


# ------------------------------------------------------------------ inputs and cached references of the prox cases
@functools.lru_cache(maxsize=None)
def images(shape, nch, n=N_IMAGES):
    """[n, nch, H, W] float32: the step image of tests/_pixel.py at a level of its own per channel (a mixed-up channel shows) plus N(0, 10) noise."""
    rng = np.random.default_rng(7000 * shape[0] + 10 * shape[1] + nch)
    x = np.stack([PX.step_image(shape, 190.0 - 40.0 * ch) for ch in range(nch)])[None] + rng.normal(0, 10, (n, nch) + shape)
    x = PX.f32(x)
    x.setflags(write=False)
    return x


def bound_from(ref64, *ref32s):
    """(e32, bound) of tests/_pixel.bound_of with e32 the largest deviation of the float32 replays (one per arithmetic form) from float64."""
    pairs = [PX.bound_of(ref64, r) for r in ref32s]
    e32 = max(p[0] for p in pairs)
    return e32, max(PX.FACTOR * e32, 2.0 * PX.ulp32(np.max(np.abs(ref64))))


@functools.lru_cache(maxsize=None)
def prox_reference(shape, nch, t, K, bounds=None):
    """(ref64, e32, bound) of the prox case: float64, and the float32 replays in the definition's form and in the kernel's."""
    x = images(shape, nch)
    r64 = vtv_prox(x.astype(np.float64), t, K, bounds=bounds)
    e32, bound = bound_from(r64, vtv_prox(x, t, K, bounds=bounds), vtv_prox(x, t, K, bounds=bounds, form="rsqrt"))
    r64.setflags(write=False)
    return r64, e32, bound


def to_device_layout(x):
    """[n, nch, H, W] -> [nch, n, H, W] (channel-major: each channel's images contiguous)."""
    return np.ascontiguousarray(np.moveaxis(x, 1, 0))
