"""Float64 reference of the weighted Gaussian data term (LMC_DATA_WL2_* in include/lmc_atomi.h, `la.L2(weights=...)`), on top of the checker
(oracle/lmc_oracle.py) and of the pieces tests/_poisson_ref.py already restates (operators, priors, the MYULA step, the SK-ROCK recursion):

    f(x) = sigma/2 sum_p w_p ((Op x)_p - y_p)^2,      grad f(x) = sigma Op^T( w * (Op x - y) ),      L_f = sigma max(w) ||Op||^2

the input recipe of the tests and the conditions on the reference alone that make the GPU comparisons discriminate: a kernel that ignores the weights,
or one that multiplies by them AFTER the adjoint (at the store), must miss the tolerance by far."""
import numpy as np

from oracle import lmc_oracle as O  # noqa: F401  (the checker: what Op, TVRef and the step are built on)
from _poisson_ref import Op, TVRef, SeparableRef, myula_step, skrock_iteration, rel, box_kernel  # noqa: F401

SIGMA_F = 1.0 / 25.0       # noise of 5 grey levels
GAMMA = 25.0
TV_WEIGHT = 0.3
TV_NITER = 10
INF = float("inf")
BOXES = [None, (0.0, INF), (0.0, 255.0)]
ENERGY_RTOL = 5e-5


class WL2Ref:
    """Checker-side data term: `.grad(x)` and `__call__(x)` on flat images (what `O.myula` hands over) or on arrays with the image on the last two axes."""

    def __init__(self, op, y, w, sigma=1.0, dtype=np.float64):
        """`dtype`: the number format every method computes in (float64 by default; float32: the device's, for the rounding scale of tests/_pixel.py)."""
        self.op, self.sigma, self.dtype = op, float(sigma), np.dtype(dtype)
        self.y = np.asarray(y, dtype=self.dtype)
        self.dims = self.y.shape
        self.w = np.broadcast_to(np.asarray(w, dtype=self.dtype), self.dims).copy()

    def _img(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return x.reshape(self.dims) if x.ndim == 1 else x

    def residual(self, x):
        return self.op.fwd(self._img(x)) - self.y

    def grad(self, x):
        return (self.dtype.type(self.sigma) * self.op.adj(self.w * self.residual(x))).reshape(np.shape(x))

    def grad_unweighted(self, x):
        """sigma Op^T (Op x - y): what a kernel that ignores the weights computes."""
        return (self.sigma * self.op.adj(self.residual(x))).reshape(np.shape(x))

    def grad_post_adjoint(self, x):
        """sigma w * Op^T (Op x - y): the WRONG order, what a kernel that multiplies at the store computes."""
        return (self.sigma * self.w * self.op.adj(self.residual(x))).reshape(np.shape(x))

    def __call__(self, x):
        v = 0.5 * self.sigma * (self.w * self.residual(x) ** 2).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v

    def unweighted_value(self, x):
        v = 0.5 * self.sigma * (self.residual(x) ** 2).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v

    def grad_lipschitz(self):
        return self.sigma * float(np.max(self.w)) * self.op.norm2_bound()


class _WithGrad:
    """`ref` with another gradient in its place (the wrong kernels of the discrimination conditions)."""

    def __init__(self, grad):
        self.grad = grad


def weights(shape, seed=11):
    """Log-uniform on [0.25, 4] with 20 % of the pixels set to 0."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(np.log(0.25), np.log(4.0), shape))
    w[rng.uniform(size=shape) < 0.2] = 0.0
    return w


def recipe(shape, n_chains=2, seed=0, op=None):
    """Five random rectangles with levels U(20, 200) on zero, y = Op img + N(0, 5^2), chain states x0 = img + N(0, 10^2), weights as `weights`.
    -> (img, op, y, w, x0 [C, H, W])"""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    img = np.zeros(shape)
    for _ in range(5):
        i0, j0 = rng.integers(0, ny - 1), rng.integers(0, nx - 1)
        i1, j1 = rng.integers(i0 + 1, ny + 1), rng.integers(j0 + 1, nx + 1)
        img[i0:i1, j0:j1] = rng.uniform(20, 200)
    if op is None:
        op = Op("blur", *box_kernel(5))
    y = op.fwd(img) + rng.normal(0, 5.0, shape)
    x0 = img[None] + rng.normal(0, 10.0, (n_chains,) + shape)
    return img, op, y, weights(shape), x0


def step_size(ref):
    return 0.5 / (ref.grad_lipschitz() + 1.0 / GAMMA)


def assert_discriminates(ref, x0, tol):
    """Conditions on the reference alone under which a comparison at `tol` tells the right kernel from one that ignores the weights or applies them
    after the adjoint.  Returns the measured figures."""
    zero = float(np.mean(ref.w == 0))
    assert zero >= 0.10, zero
    g = ref.grad(x0)
    d_unw = rel(ref.grad_unweighted(x0), g)
    assert d_unw > 100 * tol, d_unw
    d_post = None
    if ref.op.kind == "blur":
        d_post = rel(ref.grad_post_adjoint(x0), g)
        assert d_post > 100 * tol, d_post
    tau = step_size(ref)
    pg = TVRef(ref.dims, TV_WEIGHT, TV_NITER)
    xi = np.zeros_like(x0)
    want = myula_step(ref, pg, x0, tau, GAMMA, xi)
    d_steps = [rel(myula_step(_WithGrad(ref.grad_unweighted), pg, x0, tau, GAMMA, xi), want)]
    if ref.op.kind == "blur":
        d_steps.append(rel(myula_step(_WithGrad(ref.grad_post_adjoint), pg, x0, tau, GAMMA, xi), want))
    assert min(d_steps) > 30 * tol, d_steps
    f, fu = np.asarray(ref(x0)), np.asarray(ref.unweighted_value(x0))
    d_f = float(np.min(np.abs(fu - f) / np.abs(f)))
    assert d_f > 100 * ENERGY_RTOL, d_f
    return zero, d_unw, d_post, min(d_steps), d_f
