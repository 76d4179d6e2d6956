"""The second-order TGV prior (LMC_PRIOR_TGV; include/lmc_atomi.h holds the definition) restated in numpy, dtype-generic ("every routine computes in the
dtype of its input"), with the case list, the inputs and the cached references the CPU and GPU tests share.  numpy only.

    g(x) = sigma * min_w ( sum |grad x - w|_2 + alpha0 * sum |E w|_F )

`tgv_prox` is the definition's loop.  `form="kernel"` is the same loop in the arithmetic of tgv_prox_kernel -- the projection as a multiplication by
lam / sqrt(n2) where n2 > lam^2 and by nothing elsewhere (the definition divides by max(1, |z| / lam)), and the primal update on the displacement
d = u - v: d' = clip((d + s div p) * (1 / (1 + s)), lo - v, hi - v), grad ub = grad v + grad db, u = clip(v + d) at the end (the definition carries u
itself and divides by 1 + s): the second float32 replay the bound of tests/_pixel.py asks for.
`planted`: one of the faults the bound has to reject (tests/test_tgv_reference.py)."""
import functools

import numpy as np

from oracle import lmc_oracle as O
import _pixel as PX

SHAPES = [(1, 9), (9, 1), (4, 4), (5, 7), (16, 24), (33, 70), (64, 136), (97, 261)]
ALPHAS = [0.1, 0.5, 2.0]
PROX_PARAMS = [0.75, 2.5, 40.0]
N_IMAGES = 2
STEP = np.float32(1.0 / np.sqrt(12.0))          # the library's default, as it holds it
PLANTED = ("e12_once", "swap_radii", "div2_sign", "no_wbar", "clip_after", "no_cut")


def grad(x, planted=None):
    dr, dc = O.grad2d(x)
    if planted == "no_cut":             # the row difference not cut at the last row: it reads a zero past the end
        dr[..., -1, :] = -np.asarray(x)[..., -1, :]
    return dr, dc


def sym_grad(w1, w2, planted=None):
    """E w = (e11, e22, e12)."""
    e11, a = grad(w1, planted)
    b, e22 = grad(w2, planted)
    return e11, e22, w1.dtype.type(0.5) * (a + b)


def div2(q11, q22, q12):
    return O.div2d(q11, q12), O.div2d(q12, q22)


def _project(z, n2, lam, form):
    """P_lam of the components z with squared norm n2."""
    dt = n2.dtype
    one = dt.type(1)
    if form == "kernel":
        sc = np.where(n2 > lam * lam, lam * (one / np.sqrt(np.maximum(n2, dt.type(1e-30)))), one).astype(dt)
        return [c * sc for c in z]
    den = np.maximum(one, np.sqrt(n2) / lam)
    return [c / den for c in z]


def tgv_prox(v, lam1, alpha0, niter, step=STEP, bounds=None, form="div", planted=None, return_w=False, state=False):
    """prox of t g at v[..., H, W] with lam1 = t sigma: `niter` primal-dual iterations; `bounds=(lo, hi)`: every primal iterate clipped."""
    v = np.asarray(v)
    dt = v.dtype
    s = dt.type(step)
    lam1 = dt.type(np.float32(lam1))
    lam0 = dt.type(np.float32(alpha0)) * lam1
    if planted == "swap_radii":
        lam1, lam0 = lam0, lam1
    two, one = dt.type(2), dt.type(1)
    inv1s = dt.type(np.float32(1.0) / (np.float32(1.0) + np.float32(step))) if dt == np.float32 else one / (one + s)
    clip = (lambda a: a) if bounds is None else (lambda a: np.clip(a, dt.type(bounds[0]), dt.type(bounds[1])))
    inner = (lambda a: a) if planted == "clip_after" else clip
    u, ub = v.copy(), v.copy()
    if form == "kernel":
        u, ub = np.zeros_like(v), np.zeros_like(v)
        gvx, gvy = grad(v, planted)
    w1, w2, w1b, w2b, p1, p2, q11, q22, q12 = (np.zeros_like(v) for _ in range(9))
    for _ in range(niter):
        gx, gy = grad(ub, planted)
        if form == "kernel":            # ub holds the extrapolated displacement: grad ub = grad v + grad db
            gx, gy = gvx + gx, gvy + gy
        z1, z2 = p1 + s * (gx - w1b), p2 + s * (gy - w2b)
        p1, p2 = _project([z1, z2], z1 * z1 + z2 * z2, lam1, form)
        e11, e22, e12 = sym_grad(w1b, w2b, planted)
        y11, y22, y12 = q11 + s * e11, q22 + s * e22, q12 + s * e12
        m2 = y11 * y11 + y22 * y22 + (one if planted == "e12_once" else two) * (y12 * y12)
        q11, q22, q12 = _project([y11, y22, y12], m2, lam0, form)
        dp = O.div2d(p1, p2)
        if form == "kernel":            # u holds the displacement d = u - v
            un = (u + s * dp) * inv1s
            if bounds is not None and planted != "clip_after":
                un = np.clip(un, dt.type(bounds[0]) - v, dt.type(bounds[1]) - v)
        else:
            un = inner((u + s * dp + s * v) / (one + s))
        d1, d2 = div2(q11, q22, q12)
        if planted == "div2_sign":
            d1, d2 = -d1, -d2
        w1n, w2n = w1 + s * (p1 + d1), w2 + s * (p2 + d2)
        ub = two * un - u
        if planted == "no_wbar":
            w1b, w2b = w1n, w2n
        else:
            w1b, w2b = two * w1n - w1, two * w2n - w2
        u, w1, w2 = un, w1n, w2n
    if form == "kernel":
        u = clip(v + u)                 # (the displacement is inside [lo - v, hi - v]; the sum rounds once more)
    elif planted == "clip_after":
        u = clip(u)
    assert u.dtype == dt and w1.dtype == dt
    if state:
        return u, (w1, w2), (p1, p2), (q11, q22, q12)
    return (u, np.stack([w1, w2], axis=-3)) if return_w else u


def frob(e11, e22, e12):
    return np.sqrt(e11 * e11 + e22 * e22 + 2 * e12 * e12)


def primal_energy(u, w, v, lam1, alpha0):
    """1/2 |u - v|^2 + lam1 sum |grad u - w| + alpha0 lam1 sum |E w|_F per image, float64; w [..., 2, H, W]."""
    u, w, v = (np.asarray(a, dtype=np.float64) for a in (u, w, v))
    gx, gy = O.grad2d(u)
    w1, w2 = w[..., 0, :, :], w[..., 1, :, :]
    first = np.sqrt((gx - w1) ** 2 + (gy - w2) ** 2)
    second = frob(*sym_grad(w1, w2))
    return np.sum(0.5 * (u - v) ** 2 + lam1 * first + alpha0 * lam1 * second, axis=(-2, -1))


def operator_K(u, w1, w2):
    """K (u, w) = (grad u - w, E w)."""
    gx, gy = O.grad2d(u)
    return (gx - w1, gy - w2) + tuple(sym_grad(w1, w2))


def operator_Kt(p1, p2, q11, q22, q12):
    """K^T (p, q) = (-div p, -p - div2 q)."""
    d1, d2 = div2(q11, q22, q12)
    return -O.div2d(p1, p2), -p1 - d1, -p2 - d2


# ------------------------------------------------------------------ inputs and cached references
def facets(shape):
    """A two-facet affine image: two planes that meet along the middle column, inside [30, 230]."""
    H, W = shape
    i, j = np.indices(shape, dtype=np.float64)
    a = 1.0 / max(W - 1, 1)
    b = 1.0 / max(H - 1, 1)
    left = 40.0 + 260.0 * a * j + 30.0 * b * i
    right = 40.0 + 260.0 * a * (W // 2) - 120.0 * a * (j - W // 2) + 30.0 * b * i
    return np.where(j < W // 2, left, right)


@functools.lru_cache(maxsize=None)
def images(shape, n=N_IMAGES):
    """[n, H, W] float32: image 0 the two-facet affine image plus N(0, 10) noise, the others the step image of tests/_pixel.py plus the same kind of
    noise (with n = 2: one of each)."""
    rng = np.random.default_rng(9000 * shape[0] + shape[1])
    base = np.stack([facets(shape) if k == 0 else PX.step_image(shape, 190.0 - 20.0 * (k - 1)) for k in range(n)])
    x = PX.f32(base + rng.normal(0, 10, (n,) + shape))
    x.setflags(write=False)
    return x


def bound_from(ref64, *ref32s):
    """(e32, bound) of tests/_pixel.bound_of with e32 the BETTER (smaller) of the deviations of the float32 replays from float64."""
    e32 = min(PX.bound_of(ref64, r)[0] for r in ref32s)
    return e32, max(PX.FACTOR * e32, 2.0 * PX.ulp32(np.max(np.abs(ref64))))


@functools.lru_cache(maxsize=None)
def prox_reference(shape, lam, alpha0, K, bounds=None, n=N_IMAGES):
    """((u64, e32, bound), (w64, e32, bound)) of the prox case: float64, and the float32 replays in the definition's form and in the kernel's."""
    x = images(shape, n)
    u64, w64 = tgv_prox(x.astype(np.float64), lam, alpha0, K, bounds=bounds, return_w=True)
    ud, wd = tgv_prox(x, lam, alpha0, K, bounds=bounds, return_w=True)
    uk, wk = tgv_prox(x, lam, alpha0, K, bounds=bounds, form="kernel", return_w=True)
    for a in (u64, w64):
        a.setflags(write=False)
    return (u64,) + bound_from(u64, ud, uk), (w64,) + bound_from(w64, wd, wk)
