"""Float64 reference of the Huber data term (LMC_DATA_HUBER_* in include/lmc_atomi.h, `la.HuberLoss`), on top of the checker (oracle/lmc_oracle.py) and of
the pieces tests/_poisson_ref.py and tests/_wl2_ref.py already restate (operators, priors, the MYULA step, the SK-ROCK recursion, the image recipe):

    r = Op x - y,   h_d(r) = r^2 / 2 for |r| <= d, d (|r| - d / 2) otherwise,   psi_d(r) = clamp(r, -d, d)
    f(x) = sigma sum_p h_{d_p}(r_p),      grad f(x) = sigma Op^T psi_d(Op x - y),      L_f = sigma ||Op||^2

with thresholds d in [0, +inf] (0: an unobserved pixel, +inf: the plain Gaussian term there), a float32 replay through `dtype=` for the rounding scale of
tests/_pixel.py, the input recipe of the tests, the wrong kernels that the comparisons have to tell from the right one, and the conditions on the
reference alone (`assert_discriminates`) under which they do."""
import numpy as np

from oracle import lmc_oracle as O  # noqa: F401  (the checker: what Op, TVRef and the step are built on)
from _poisson_ref import Op, TVRef, SeparableRef, myula_step, skrock_iteration, rel, box_kernel  # noqa: F401
import _wl2_ref as W
from _wl2_ref import SIGMA_F, GAMMA, TV_WEIGHT, TV_NITER, INF, BOXES, ENERGY_RTOL, step_size, _WithGrad  # noqa: F401

STEP_TOL = 1e-5


def f32(a):
    """Rounded to float32 once, as float64: the numbers the library gets."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def psi(r, d):
    """clamp(r, -d, d), exact in any format (it returns one of its operands); d = +inf passes r through, d = 0 gives 0."""
    return np.minimum(np.maximum(r, -d), d)


def huber(r, d):
    """h_d(r), elementwise.  d = +inf takes the quadratic branch (no inf * 0 is formed), d = 0 the linear one, which gives 0."""
    a = np.abs(r)
    quad = a <= d
    dl = np.where(quad, 0, d)       # (finite where the linear branch is taken)
    return np.where(quad, a * a / 2, dl * (a - dl / 2))


class HuberRef:
    """Checker-side data term: `.grad(x)` and `__call__(x)` on flat images (what `O.myula` hands over) or on arrays with the image on the last two axes."""

    def __init__(self, op, y, delta, sigma=1.0, dtype=np.float64):
        """`dtype`: the number format every method computes in (float64 by default; float32: the device's, for the rounding scale of tests/_pixel.py)."""
        self.op, self.sigma, self.dtype = op, float(sigma), np.dtype(dtype)
        self.y = np.asarray(y, dtype=self.dtype)
        self.dims = self.y.shape
        self.delta = np.broadcast_to(np.asarray(delta, dtype=self.dtype), self.dims).copy()

    def _img(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return x.reshape(self.dims) if x.ndim == 1 else x

    def fwd(self, x):
        return self.op.fwd(self._img(x))

    def residual(self, x):
        return self.fwd(x) - self.y

    def _adj(self, d, x):
        return (self.dtype.type(self.sigma) * self.op.adj(d)).reshape(np.shape(x))

    def grad(self, x):
        return self._adj(psi(self.residual(x), self.delta), x)

    def __call__(self, x):
        v = self.sigma * huber(self.residual(x), self.delta).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v

    def grad_lipschitz(self):
        return self.sigma * self.op.norm2_bound()

    def clipped(self, x):
        """Share of the pixels whose residual lies outside [-delta, delta] (delta = 0 pixels included)."""
        return float(np.mean(np.abs(self.residual(x)) > self.delta))

    # -- the wrong kernels ------------------------------------------------------------------------------------------------
    def grad_plain(self, x):
        """sigma Op^T (Op x - y): delta ignored, the plain Gaussian term."""
        return self._adj(self.residual(x), x)

    def grad_post_adjoint(self, x):
        """sigma clamp(Op^T (Op x - y), -delta, delta): the clamp AFTER the adjoint, at the store."""
        return (self.sigma * psi(self.op.adj(self.residual(x)), self.delta)).reshape(np.shape(x))

    def grad_clamp_of_hx(self, x):
        """sigma Op^T (clamp(Op x, -delta, delta) - y): the clamp on Op x instead of the residual."""
        return self._adj(psi(self.fwd(x), self.delta) - self.y, x)

    def grad_planes_swapped(self, x):
        """sigma Op^T clamp(Op x - delta, -y, y): plane 1 read as the observation, plane 0 as the threshold."""
        with np.errstate(invalid="ignore"):
            return self._adj(psi(self.fwd(x) - self.delta, self.y), x)

    def grad_times_delta(self, x):
        """sigma Op^T (delta * (Op x - y)): the threshold plane used as WL2 uses its weights."""
        with np.errstate(invalid="ignore"):
            return self._adj(self.delta * self.residual(x), x)

    def plain_value(self, x):
        """sigma / 2 sum (Op x - y)^2: the value of the plain Gaussian term."""
        v = 0.5 * self.sigma * (self.residual(x) ** 2).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v

    def value_without_offset(self, x):
        """The linear branch as delta |r|, without - delta^2 / 2: not continuous at |r| = delta."""
        r, d = np.abs(self.residual(x)), self.delta
        quad = r <= d
        v = self.sigma * np.where(quad, r * r / 2, np.where(quad, 0, d) * r).sum(axis=(-2, -1))
        return float(v) if np.ndim(v) == 0 else v


def thresholds(shape, seed=13):
    """Log-uniform on [3, 12], 10 % of the pixels set to 0 and another 10 % to +inf."""
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(3.0), np.log(12.0), shape))
    u = rng.uniform(size=shape)
    d[u < 0.1] = 0.0
    d[(u >= 0.1) & (u < 0.2)] = INF
    return d


def recipe(shape, n_chains=2, seed=0, op=None):
    """`_wl2_ref.recipe` (five rectangles, y = Op img + N(0, 5^2), x0 = img + N(0, 10^2)) with outliers +-U(50, 150) on 10 % of y and thresholds as
    `thresholds`; every array rounded to float32 once, so that the library and the reference start from the same numbers.
    -> (img, op, y, delta, x0 [C, H, W])"""
    img, op, y, _, x0 = W.recipe(shape, n_chains=n_chains, seed=seed, op=op)
    rng = np.random.default_rng(5)
    hit = rng.uniform(size=shape) < 0.1
    amp = rng.uniform(50.0, 150.0, shape) * rng.choice([-1.0, 1.0], shape)
    y = y + np.where(hit, amp, 0.0)
    if op.kind == "blur":
        op = Op("blur", f32(op.args[0]), op.args[1])        # (the device operator keeps its taps in float32)
    return img, op, f32(y), f32(thresholds(shape)), f32(x0)


def wrong_gradients(ref):
    """name -> the gradient of a wrong kernel; the clamp after the adjoint only differs in kind under a blur (the identity's adjoint is the identity)."""
    out = {"delta ignored": ref.grad_plain, "clamp of Op x": ref.grad_clamp_of_hx, "planes swapped": ref.grad_planes_swapped,
           "times delta": ref.grad_times_delta}
    if ref.op.kind == "blur":
        out["clamp after the adjoint"] = ref.grad_post_adjoint
    return out


def distance(a, b):
    """rel-L2 of a against b; +inf where a is not finite (a wrong kernel that meets delta = +inf)."""
    return rel(a, b) if np.isfinite(a).all() else INF


def assert_discriminates(ref, x0, tol=STEP_TOL):
    """Conditions on the reference alone under which a comparison at `tol` tells the right kernel from the wrong ones.  Returns the measured figures:
    (clipped share, delta = 0 share, delta = inf share, {wrong gradient: rel-L2}, least rel-L2 of a wrong step, least relative distance of the L2 value)."""
    clipped, zero, inf = ref.clipped(x0), float(np.mean(ref.delta == 0)), float(np.mean(np.isinf(ref.delta)))
    assert 0.2 <= clipped <= 0.8, clipped
    assert zero >= 0.05 and inf >= 0.05, (zero, inf)
    g = ref.grad(x0)
    d_grad = {name: distance(fn(x0), g) for name, fn in wrong_gradients(ref).items()}
    assert min(d_grad.values()) > 100 * tol, d_grad
    tau = step_size(ref)
    pg = TVRef(ref.dims, TV_WEIGHT, TV_NITER)
    xi = np.zeros_like(x0)
    want = myula_step(ref, pg, x0, tau, GAMMA, xi)
    d_steps = [distance(myula_step(_WithGrad(fn), pg, x0, tau, GAMMA, xi), want) for fn in wrong_gradients(ref).values()]
    assert min(d_steps) > 30 * tol, d_steps
    f, fp = np.asarray(ref(x0)), np.asarray(ref.plain_value(x0))
    d_f = float(np.min(np.abs(fp - f) / np.abs(f)))
    assert d_f > 100 * ENERGY_RTOL, d_f
    return clipped, zero, inf, d_grad, min(d_steps), d_f
