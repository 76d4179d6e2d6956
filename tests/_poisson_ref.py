"""Float64 reference of the Poisson data term (LMC_DATA_POISSON_* in include/lmc_atomi.h, `la.Poisson`), on top of the checker (oracle/lmc_oracle.py):
the definition restated, a checker-side data-term object for `O.myula`, the SK-ROCK recursion of the header text, the input recipe of the tests and
the conditions on the reference alone that make the GPU comparisons discriminate.

    u >= 0:  phi(u) = (u + beta) - y + y log(y / (u + beta))      (0 log 0 = 0)       phi'(u) = 1 - y / (u + beta)
    u <  0:  phi(u) = phi(0) + phi'(0) u + y u^2 / (2 beta^2)                          phi'(u) = 1 - y / beta + y u / beta^2
    f(x) = sigma sum_p phi_p((Op x)_p),      grad f(x) = sigma Op^T phi'(Op x)

Everything computes in float64 unless a `dtype` is handed in (`dtype=np.float32`: the same operations in the device's number format, whose distance from
the float64 result is the rounding scale of tests/_pixel.py); the float64 results do not depend on the keyword being there.
"""
import numpy as np
from numpy.polynomial import chebyshev as cheb

from oracle import lmc_oracle as O


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# ------------------------------------------------------------------ the definition
def _kl(d, y):
    """d - y + y log(y / d) with 0 log 0 = 0, d > 0"""
    one, zero = d.dtype.type(1), d.dtype.type(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ylog = np.where(y > 0, y * np.log(np.where(y > 0, y, one) / d), zero)
    return d - y + ylog


def phi(u, y, beta, dtype=np.float64):
    u, y, beta = np.broadcast_arrays(np.asarray(u, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(beta, dtype=dtype))
    one, two, zero = u.dtype.type(1), u.dtype.type(2), u.dtype.type(0)
    pos = _kl(np.maximum(u, zero) + beta, y)
    neg = _kl(beta, y) + (one - y / beta) * u + y * u * u / (two * beta * beta)
    return np.where(u >= 0, pos, neg)


def dphi(u, y, beta, dtype=np.float64):
    u, y, beta = np.broadcast_arrays(np.asarray(u, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(beta, dtype=dtype))
    one, zero = u.dtype.type(1), u.dtype.type(0)
    return np.where(u >= 0, one - y / (np.maximum(u, zero) + beta), one - y / beta + y * u / (beta * beta))


def dphi_unextended(u, y, beta):
    """The Kullback-Leibler derivative used below 0 as well: what a kernel that drops the second branch computes."""
    return 1.0 - np.asarray(y) / (np.asarray(u) + np.asarray(beta))


class Op:
    """The three operators of the data term on images (last two axes): ('blur', h, offset) | ('mask', m) | ('identity',)."""

    def __init__(self, kind, *args):
        self.kind, self.args = kind, args

    def fwd(self, x):
        if self.kind == "blur":
            return O.blur(x, self.args[0], self.args[1])
        return x * np.asarray(self.args[0], dtype=x.dtype) if self.kind == "mask" else x

    def adj(self, r):
        if self.kind == "blur":
            return O.blur_adjoint(r, self.args[0], self.args[1])
        return r * np.asarray(self.args[0], dtype=r.dtype) if self.kind == "mask" else r

    def norm2_bound(self):
        return float(np.abs(self.args[0]).sum()) ** 2 if self.kind == "blur" else 1.0


class PoissonRef:
    """Checker-side data term: `.grad(x)` and `__call__(x)` on flat images (what `O.myula` hands over) or on arrays with the image on the last two axes."""

    def __init__(self, op, y, beta, sigma=1.0, dtype=np.float64):
        self.op, self.sigma, self.dtype = op, float(sigma), np.dtype(dtype)
        self.y = np.asarray(y, dtype=self.dtype)
        self.dims = self.y.shape
        self.beta = np.broadcast_to(np.asarray(beta, dtype=self.dtype), self.dims).copy()

    def _img(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return x.reshape(self.dims) if x.ndim == 1 else x

    def u(self, x):
        return self.op.fwd(self._img(x))

    def grad(self, x):
        g = self.dtype.type(self.sigma) * self.op.adj(dphi(self.u(x), self.y, self.beta, dtype=self.dtype))
        return g.reshape(np.shape(x))

    def grad_with(self, x, rho):
        """The gradient with another pointwise functor in place of phi' (the wrong kernels of the discrimination conditions)."""
        return self.sigma * self.op.adj(rho(self.u(x), self.y, self.beta))

    def __call__(self, x):
        v = self.sigma * phi(self.u(x), self.y, self.beta, dtype=self.dtype).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v

    def grad_lipschitz(self):
        return self.sigma * float(np.max(self.y / self.beta ** 2)) * self.op.norm2_bound()


# ------------------------------------------------------------------ priors of the checker (the prox of O.myula's proxg)
def tv_prox_box(x, gamma, niter, lo=-np.inf, hi=np.inf, aniso=False, step=0.125, dtype=np.float64):
    """prox of gamma TV (either form) + the indicator of [lo, hi]: the checker's fast gradient projection with the primal iterate clipped in every dual
    iteration and on return (Beck and Teboulle), as tests/test_gpu_tv_box.py restates it; an infinite box is the checker's `O.tv_prox_fgp`."""
    x = np.asarray(x, dtype=dtype)
    dt = x.dtype.type
    gamma, lo, hi, one = dt(gamma), dt(lo), dt(hi), dt(1)
    c = dt(step) / gamma
    betas = np.asarray(O.fgp_betas(niter, "unlocbox"), dtype=x.dtype)
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    for k in range(niter):
        dr, dc = O.grad2d(np.clip(x - gamma * O.div2d(rr, ss), lo, hi))
        r, s = rr - c * dr, ss - c * dc
        if aniso:
            pn, qn = np.clip(r, -one, one), np.clip(s, -one, one)
        else:
            n = np.maximum(one, np.sqrt(r * r + s * s))
            pn, qn = r / n, s / n
        rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
        p, q = pn, qn
    return np.clip(x - gamma * O.div2d(rr, ss), lo, hi)


class TVRef:
    def __init__(self, dims, sigma, niter, bounds=None, aniso=False, dtype=np.float64):
        self.dims, self.sigma, self.niter, self.aniso, self.dtype = dims, sigma, niter, aniso, np.dtype(dtype)
        self.lo, self.hi = bounds if bounds is not None else (-np.inf, np.inf)

    def prox(self, x, t):
        x = np.asarray(x)
        img = x.reshape(self.dims) if x.ndim == 1 else x
        return tv_prox_box(img, self.sigma * t, self.niter, self.lo, self.hi, aniso=self.aniso, dtype=self.dtype).reshape(x.shape)

    def value(self, x):
        dr, dc = O.grad2d(np.asarray(x, dtype=np.float64))
        return (np.abs(dr) + np.abs(dc) if self.aniso else np.sqrt(dr * dr + dc * dc)).sum(axis=(-2, -1))


class SeparableRef:
    """clip(closed-form prox)"""

    def __init__(self, prox, bounds=None, dtype=np.float64):
        self._prox, self.dtype = prox, np.dtype(dtype)
        self.lo, self.hi = bounds if bounds is not None else (-np.inf, np.inf)

    def prox(self, x, t):
        return np.clip(self._prox(np.asarray(x, dtype=self.dtype), t), self.dtype.type(self.lo), self.dtype.type(self.hi))


def myula_step(pf, pg, x, tau, gamma, xi, dtype=None):
    """One MYULA step on arrays with the image on the last two axes (algs.py:569).  `dtype=None`: as numpy promotes the operands (float64 from float64
    terms); a dtype: state, noise and the four coefficients in it (the terms `pf` and `pg` are built with the same one)."""
    if dtype is None:
        return (1 - tau / gamma) * x - tau * pf.grad(x) + tau / gamma * pg.prox(x, gamma) + np.sqrt(2 * tau) * xi
    dt = np.dtype(dtype).type
    x, xi = np.asarray(x, dtype=dtype), np.asarray(xi, dtype=dtype)
    return dt(1 - tau / gamma) * x - dt(tau) * pf.grad(x) + dt(tau / gamma) * pg.prox(x, gamma) + dt(np.sqrt(2 * tau)) * xi


# ------------------------------------------------------------------ SK-ROCK, restated from the header text of lmc_skrock_create
def skrock_coefficients(s, eta):
    T = lambda j, x: cheb.chebval(x, [0.0] * j + [1.0])
    dT = lambda j, x: cheb.chebval(x, cheb.chebder([0.0] * j + [1.0]))
    w0 = 1.0 + eta / s ** 2
    w1 = T(s, w0) / dT(s, w0)
    mu = [w1 / w0] + [2 * w1 * T(j - 1, w0) / T(j, w0) for j in range(2, s + 1)]
    nu = [s * w1 / 2] + [2 * w0 * T(j - 1, w0) / T(j, w0) for j in range(2, s + 1)]
    kappa = [s * w1 / w0] + [-T(j - 2, w0) / T(j, w0) for j in range(2, s + 1)]
    return np.array(mu), np.array(nu), np.array(kappa)


def skrock_iteration(pf, pg, x, Z, delta, gamma, s, eta=0.05):
    """K_0 = X, K_1 = X + mu_1 delta drift(X + nu_1 q Z) + kappa_1 q Z, K_j = mu_j delta drift(K_{j-1}) + nu_j K_{j-1} + kappa_j K_{j-2}; q = sqrt(2 delta),
    drift(x) = -grad f(x) - (x - prox_{gamma g}(x)) / gamma."""
    drift = lambda v: -pf.grad(v) - (v - pg.prox(v, gamma)) / gamma
    mu, nu, kappa = skrock_coefficients(s, eta)
    q = np.sqrt(2 * delta)
    k2, k1 = x, x + mu[0] * delta * drift(x + nu[0] * q * Z) + kappa[0] * q * Z
    for j in range(2, s + 1):
        k1, k2 = mu[j - 1] * delta * drift(k1) + nu[j - 1] * k1 + kappa[j - 1] * k2, k1
    return k1


# ------------------------------------------------------------------ the input recipe
def box_kernel(k):
    return np.ones((k, k)) / (k * k), (k // 2, k // 2)


def ramp_background(shape):
    """The array-valued background of the tests: a ramp from 0.3 to 1.0 along the rows' direction."""
    return np.broadcast_to(np.linspace(0.3, 1.0, shape[1])[None, :], shape).copy()


def recipe(shape, n_chains=2, seed=0, k=5, beta=0.5, op=None):
    """Five random rectangles with levels U(2, 30) on a zero background, y = Poisson(Op img + beta), chain states x0 = img + N(0, 2^2) - 1.5.
    `op`: an `Op` (default: the k x k box blur); `beta`: a scalar or an [H, W] array.  -> (img, op, y, beta [H, W], x0 [C, H, W])"""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    img = np.zeros(shape)
    for _ in range(5):
        i0, j0 = rng.integers(0, ny - 1), rng.integers(0, nx - 1)
        i1, j1 = rng.integers(i0 + 1, ny + 1), rng.integers(j0 + 1, nx + 1)
        img[i0:i1, j0:j1] = rng.uniform(2, 30)
    if op is None:
        op = Op("blur", *box_kernel(k))
    beta = np.broadcast_to(np.asarray(beta, dtype=np.float64), shape).copy()
    y = rng.poisson(op.fwd(img) + beta).astype(np.float64)
    x0 = img[None] + rng.normal(0, 2.0, (n_chains,) + shape) - 1.5
    return img, op, y, beta, x0


def random_mask(shape, seed=5):
    return (np.random.default_rng(seed).uniform(size=shape) < 0.6).astype(np.float64)


def gaussian_grad(pf, x):
    """sigma Op^T (Op x - y): what a kernel that keeps the old residual computes."""
    return pf.grad_with(x, lambda u, y, beta: u - y)


def coverage(pf, x):
    """(fraction of pixels with y = 0, with u < 0, with u > 0, sum |phi| / |sum phi|) of the states x"""
    u = pf.u(x)
    p = phi(u, pf.y, pf.beta)
    return float(np.mean(pf.y == 0)), float(np.mean(u < 0)), float(np.mean(u > 0)), float(np.abs(p).sum() / abs(p.sum()))


def assert_discriminates(pf, x, tol):
    """The conditions on the reference alone under which a comparison at `tol` tells the right kernel from one that drops a branch of phi' or keeps the
    Gaussian residual."""
    y0, neg, pos, cond = coverage(pf, x)
    assert y0 >= 0.10 and neg >= 0.10 and pos >= 0.10, (y0, neg, pos)
    assert cond <= 2.0, cond
    g = pf.grad(x)
    d_unext, d_gauss = rel(pf.grad_with(x, dphi_unextended), g), rel(gaussian_grad(pf, x), g)
    assert d_unext > 100 * tol and d_gauss > 100 * tol, (d_unext, d_gauss)
    return y0, neg, pos, cond, d_unext, d_gauss
