"""GPU parity of the box-constrained priors, g(x) + the indicator of lo <= x <= hi, as `bounds=(lo, hi)`: the TV prox alone (pipe kernels
`myula_step_pipe_box_kernel` / `myula_step_pipe_box2_kernel`, tile kernel `myula_step_tile_box_kernel`), both forms of the prior, inside the fused MYULA
step, the separable priors (`L1`, `L2`, the closed forms, `Box` alone), and the refusals of the C ABI and of the Python surface.

The reference of the TV prox is `tv_prox_box` below: the checker's fast gradient projection (`O.tv_prox_fgp`, oracle/lmc_oracle.py) with ONE change --
the primal iterate is clipped to the box inside every dual iteration and on return (Beck and Teboulle's constrained FGP).  With infinite bounds it equals
`O.tv_prox_fgp` bit for bit; it converges to the prox of the sum, which "clip afterwards" does not: every discriminating case first asserts, on the
reference alone, that the two differ by far more than the tolerance, so that a kernel that clamps only at the end (or not at all) fails.

Tolerances are the project's (tests/test_gpu_parity.py): one operator / one step rel-L2 <= 1e-5, and 1e-5 x (step index) along a trajectory.  Two of the
three boxes exclude 0: pixels outside the image (lanes past W, rows outside, vacant lanes of a wave shift) hold 0 before the clamp and lo or hi after it,
so a difference that is cut by the fill value being 0 rather than by an edge coefficient shows up as an error along the image edges.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
TAU_REG = 0.3
INF = float("inf")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def tv_prox_box(x, gamma, niter, lo, hi, aniso=False, step=0.125, momentum="unlocbox"):
    """prox of gamma TV + the indicator of [lo, hi]: `niter` FGP dual updates from the zero dual, the primal iterate clipped in every one of them and on
    return; images on the last two axes."""
    x = np.asarray(x)
    dt = x.dtype
    gamma = dt.type(gamma)
    c = dt.type(step) / gamma
    betas = np.asarray(O.fgp_betas(niter, momentum), dtype=dt)
    rr, ss, p, q = (np.zeros_like(x) for _ in range(4))
    one = dt.type(1)
    lo, hi = dt.type(lo), dt.type(hi)
    for k in range(niter):
        sol = np.clip(x - gamma * O.div2d(rr, ss), lo, hi)            # <- the only change (k = 0: clip(x))
        dr, dc = O.grad2d(sol)
        r, s = rr - c * dr, ss - c * dc
        if aniso:
            pn, qn = np.clip(r, -one, one), np.clip(s, -one, one)
        else:
            n = np.maximum(one, np.sqrt(r * r + s * s))
            pn, qn = r / n, s / n
        rr, ss = pn + betas[k] * (pn - p), qn + betas[k] * (qn - q)
        p, q = pn, qn
    return np.clip(x - gamma * O.div2d(rr, ss), lo, hi)               # <- and the returned iterate


def tv_prox_free(x, gamma, niter, aniso=False, momentum="unlocbox"):
    """The unconstrained prox of either form: the same loop with an infinite box."""
    return tv_prox_box(x, gamma, niter, -INF, INF, aniso=aniso, momentum=momentum)


def test_reference_with_an_infinite_box_is_the_checkers_prox():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(2, 20, 33)) * 40 + 100
    for momentum in ("unlocbox", "fista"):
        np.testing.assert_array_equal(tv_prox_free(x, 15.0, 10, momentum=momentum), O.tv_prox_fgp(x, 15.0, 10, momentum=momentum))


class BoxTV:
    """The checker-side prior object (what O.myula calls)."""

    def __init__(self, dims, sigma, niter, lo, hi, aniso=False):
        self.dims, self.sigma, self.niter, self.lo, self.hi, self.aniso = dims, sigma, niter, lo, hi, aniso

    def prox(self, x, t):
        return tv_prox_box(np.asarray(x).reshape(self.dims), self.sigma * t, self.niter, self.lo, self.hi, aniso=self.aniso).ravel()


class Clipped:
    """Checker-side separable prior: the clamp of a closed-form prox (exact for a separable g); `t` may be an array (array-valued epsg)."""

    def __init__(self, prox, lo, hi):
        self._prox, self.lo, self.hi = prox, lo, hi

    def prox(self, x, t):
        return np.clip(self._prox(np.asarray(x), t), self.lo, self.hi)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


def synth(ny, nx, seed=0, k=5, sigma=0.75):
    rng = np.random.default_rng(seed)
    img = np.zeros((ny, nx))
    for _ in range(5):
        i0, j0 = rng.integers(0, ny - 1), rng.integers(0, nx - 1)
        i1, j1 = rng.integers(i0 + 1, ny + 1), rng.integers(j0 + 1, nx + 1)
        img[i0:i1, j0:j1] = rng.uniform(20, 235)
    img += np.linspace(0, 20, nx)[None, :]
    h = np.ones((k, k)) / (k * k)
    y = O.blur(img, h, (k // 2, k // 2)) + rng.normal(0, sigma, (ny, nx))
    return img, h, y


@functools.lru_cache(maxsize=None)
def prox_input(shape, shift):
    """The image a prox case works on (levels 20 - 235 plus N(0, 8)), computed once per shape; `shift` moves it under the box (-60, -10)."""
    img, _, _ = synth(*shape, seed=1)
    x = img + np.random.default_rng(shape[1]).normal(0, 8, shape) + shift
    x.setflags(write=False)
    return x


BOXES = [(40.0, 200.0, 0.0), (0.0, 255.0, 0.0), (-60.0, -10.0, -150.0)]      # (lo, hi, shift of the image)
DISCRIMINATING = {(40.0, 200.0), (-60.0, -10.0)}

# (niter, shape, lagged_output, which kernel, prox parameters): every instantiation family of the pipe kernel and every reason for the tile kernel
PROX_CASES = [
    (10, (16, 16), False, "tile", (15.0, 0.16875)),          # W <= 128
    (10, (40, 136), False, "pipe", (15.0,)),                 # PXL 4, aligned
    (10, (33, 203), False, "pipe", (15.0, 0.16875)),         # PXL 4, unaligned
    (10, (24, 264), False, "pipe", (15.0,)),                 # PXL 8
    (10, (24, 877), False, "pipe", (15.0, 0.16875)),         # two strips, unaligned
    (10, (33, 520), False, "pipe", (15.0,)),                 # strips at an aligned width
    (10, (16, 1544), False, "pipe", (15.0,)),                # four strips
    (20, (64, 136), False, "pipe", (15.0,)),                 # chain links, PXL 4
    (50, (40, 200), False, "pipe", (15.0,)),                 # chain links, five of them
    (9, (40, 96), False, "tile", (15.0,)),
    (9, (40, 96), True, "tile", (15.0,)),                    # lagged_output: niter = 10 asked for, the iterate after 9 updates returned
    (6, (33, 520), False, "tile", (15.0,)),                  # a count the pipe does not cover, on a wide image
    (17, (40, 96), False, "tile", (15.0,)),                  # above 12: chunks of 8 + 8 + 1 chained through the dual state; a resumed chunk first clamps x - gamma div(state)
]
# strip seams of the one-team pipe kernel at 8 pixels per lane without a blur: strips of 512 columns with halos of 16, so 480 written columns each
SEAMS = {877: (480,), 520: (480,), 1544: (480, 960, 1440)}


def check_seams(got, ref, W, what):
    """Column-wise: nothing special at the strip seams (tests/test_gpu_wide.py).  Every column runs the same arithmetic, so the worst error of the few seam
    columns stays within a small factor of the worst over the hundreds of interior columns (+ two ulps of 255 in float32 of slack), and within the 2e-3 of
    test_gpu_wide."""
    colerr = np.abs(np.asarray(got, dtype=np.float64) - ref).reshape(-1, ref.shape[-2], W).max(axis=(0, 1))
    seam = np.zeros(W, dtype=bool)
    for s in SEAMS[W]:
        seam[s - 2:s + 2] = True
    seam[-2:] = True                   # and the last image columns
    s_max, i_max = float(colerr[seam].max()), float(colerr[~seam].max())
    print(f"  {what}: column-wise max error at the seams {s_max:.3e}, interior {i_max:.3e}")
    assert s_max < 2e-3 and s_max <= 4 * i_max + 6e-5, (s_max, i_max)


@pytest.mark.parametrize("niter,shape,lagged,kernel,params", PROX_CASES)
def test_box_prox_matches_reference(la, niter, shape, lagged, kernel, params):
    for lo, hi, shift in BOXES:
        x = prox_input(shape, shift)
        for par in params:
            for momentum in ("unlocbox", "fista"):
                ref = tv_prox_box(x, par, niter, lo, hi, momentum=momentum)
                if par == 15.0:        # the condition on the reference alone (0.16875 is the MYULA regime: there for parity, not for discrimination)
                    free = tv_prox_free(x, par, niter, momentum=momentum)
                    d_clip, d_free = rel(np.clip(free, lo, hi), ref), rel(free, ref)
                    print(f"reference niter={niter} {shape} box=({lo}, {hi}) {momentum}: vs clip-after {d_clip:.2e}, vs unconstrained {d_free:.2e}")
                    if (lo, hi) in DISCRIMINATING:
                        assert d_clip >= 1e-4 and d_free >= 1e-2, (d_clip, d_free)
                tv = la.TV(shape, sigma=TAU_REG, niter=niter + 1 if lagged else niter, momentum=momentum, lagged_output=lagged, bounds=(lo, hi))
                out = tv.prox(x.ravel(), par / TAU_REG)
                assert out.shape == (shape[0] * shape[1],)
                e = rel(out, ref.ravel())
                print(f"prox niter={niter} {shape} box=({lo}, {hi}) parameter {par} {momentum}: rel {e:.3e}")
                assert e < STEP_TOL, (lo, hi, par, momentum, e)
                assert out.min() >= np.float32(lo) and out.max() <= np.float32(hi), (out.min(), out.max())
                if shape[1] in SEAMS and kernel == "pipe":
                    check_seams(out.reshape(shape), ref, shape[1], f"box=({lo}, {hi})")
    # the value is that of the TV term alone: the indicator is not reported
    tv = la.TV(shape, sigma=TAU_REG, niter=niter, bounds=(40.0, 200.0))
    x = prox_input(shape, 0.0)
    val, vref = tv(x.ravel()), TAU_REG * float(O.tv_value(x))
    assert abs(val - vref) <= 1e-5 * vref


def test_box_prox_batch_and_kernel_names(la):
    """A batch of images through `prox`, and the kernel a sampler reports for each family."""
    x = np.stack([prox_input((24, 264), 0.0)] * 3) + np.arange(3)[:, None, None]
    out = la.TV((24, 264), sigma=1.0, niter=10, bounds=(40, 200)).prox(x, 15.0)
    assert out.shape == x.shape
    assert rel(out, tv_prox_box(x, 15.0, 10, 40.0, 200.0)) < STEP_TOL
    for shape, niter, iso, want in [((24, 264), 10, True, "myula_step_pipe_box_kernel"), ((24, 96), 10, True, "myula_step_tile_box_kernel"),
                                    ((24, 264), 7, True, "myula_step_tile_box_kernel"), ((24, 264), 10, False, "myula_step_tile_box_kernel")]:
        smp = la.MYULASampler(None, la.TV(shape, sigma=TAU_REG, niter=niter, isotropic=iso, bounds=(40, 200)), shape, n_chains=2, tau=0.1, gamma=0.5)
        smp.set_state(prox_input(shape, 0.0))
        smp.step(1)
        assert smp.kernel_name == want, (shape, niter, iso, smp.kernel_name)
        smp.close()


# ------------------------------------------------------------------ 2. anisotropic prior + box (tile kernel at every width)
@pytest.mark.parametrize("shape,niter", [((16, 16), 10), ((40, 264), 10), ((24, 877), 10), ((33, 203), 17)])      # 17: chunks of 8 + 8 + 1 through the dual state
def test_aniso_box_prox_matches_reference(la, shape, niter):
    par = 15.0
    for lo, hi, shift in BOXES:
        x = prox_input(shape, shift)
        ref = tv_prox_box(x, par, niter, lo, hi, aniso=True)
        free = tv_prox_free(x, par, niter, aniso=True)
        d_clip = rel(np.clip(free, lo, hi), ref)
        print(f"reference (anisotropic) {shape} box=({lo}, {hi}): vs clip-after {d_clip:.2e}, vs unconstrained {rel(free, ref):.2e}")
        if (lo, hi) == (40.0, 200.0):
            assert d_clip >= 1e-4, d_clip
        out = la.TV(shape, sigma=TAU_REG, niter=niter, isotropic=False, bounds=(lo, hi)).prox(x.ravel(), par / TAU_REG)
        e = rel(out, ref.ravel())
        print(f"anisotropic prox {shape} niter={niter} box=({lo}, {hi}): rel {e:.3e}")
        assert e < STEP_TOL, (lo, hi, e)
        assert out.min() >= np.float32(lo) and out.max() <= np.float32(hi)


# ------------------------------------------------------------------ 3. fused MYULA step, injected noise
def build(la, data, k, shape, rng, sigma, ncvx=False):
    """(x0 base image, device data term, checker data term)"""
    img, h, y = synth(*shape, seed=2, k=max(k, 3), sigma=sigma)
    if data == "blur":
        off = (k // 2, k // 2)
        Op, oOp = la.Convolve2D(shape, h, offset=off), O.Convolve2D(shape, h, off)
    elif data == "identity":
        y = img + rng.normal(0, sigma, shape)
        Op, oOp = None, None
    else:
        mask = (rng.uniform(size=shape) < 0.5).astype(np.float64)
        y = mask * img + rng.normal(0, sigma, shape) * mask
        Op, oOp = la.Diagonal(mask, dims=shape), O.Diagonal(mask)
    if ncvx:
        kw = dict(dims=shape, b=y.ravel(), sigma=1 / sigma ** 2, lamda=0.3, gamma=15.0, isotropic=True, niter=20)
        return img, la.L2_ncvx_tv(Op=Op, Op2=la.Gradient(shape), **kw), O.L2NcvxTV(Op=oOp, Op2=O.Gradient(shape), **kw)
    return img, la.L2(Op=Op, b=y.ravel(), sigma=1 / sigma ** 2, dims=shape), O.L2(Op=oOp, b=y.ravel(), sigma=1 / sigma ** 2)


def pipe_covers(W, niter):
    return W > 128 and niter % 10 == 0 and 10 <= niter <= 60


# noise sigma 6: the prox parameter 0.3 sigma^2 = 10.8 is in the regime where the in-loop clamp matters; 0.75 is the project's
STEP_CASES = [("blur", 5, (24, 96), 10, 6.0), ("blur", 5, (24, 136), 10, 6.0), ("blur", 7, (24, 264), 10, 6.0), ("blur", 5, (24, 520), 10, 6.0),
              ("blur", 7, (24, 877), 10, 6.0), ("identity", 0, (24, 264), 10, 6.0), ("identity", 0, (24, 877), 10, 6.0), ("mask", 0, (25, 136), 10, 6.0),
              ("mask", 0, (24, 520), 10, 6.0), ("blur", 5, (24, 264), 10, 0.75), ("blur", 5, (24, 877), 10, 0.75), ("identity", 0, (24, 96), 10, 0.75),
              ("mc", 5, (24, 264), 10, 6.0), ("blur", 5, (24, 264), 20, 6.0)]


@pytest.mark.parametrize("data,k,shape,niter,sigma", STEP_CASES)
def test_myula_steps_box_injected_noise(la, data, k, shape, niter, sigma):
    rng = np.random.default_rng(11)
    C_, nit = 3, 6
    lo, hi = 40.0, 200.0
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    img, pf, of = build(la, "blur" if data == "mc" else data, k, shape, rng, sigma, ncvx=data == "mc")
    pg, og = la.TV(shape, sigma=TAU_REG, niter=niter, bounds=(lo, hi)), BoxTV(shape, TAU_REG, niter, lo, hi)
    x0 = img[None] + rng.normal(0, 10, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=gamma, noise="injected")
    smp.set_state(x0)
    ref = np.stack([O.myula(of, og, x0[c].ravel(), tau, gamma, niter=nit, noise=[noise[i, c].ravel() for i in range(nit)]).reshape((nit,) + shape)
                    for c in range(C_)], axis=1)        # [nit, C, H, W]
    for it in range(nit):
        smp.step(1, noise=noise[it:it + 1])
        got = smp.get_state().cpu().numpy()
        e = rel(got, ref[it])
        print(f"{data} k={k} {shape} niter={niter} sigma={sigma} step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    assert ("pipe_box" if pipe_covers(shape[1], niter) else "tile_box") in smp.kernel_name, smp.kernel_name
    smp.close()


# ------------------------------------------------------------------ 4. Philox path: one team and two teams
def test_one_team_and_two_team_box_kernels_are_bit_identical(la):
    """Every pixel runs the one-team kernel's arithmetic on the same operands; auto picks the two-team layout here."""
    shape = (40, 512)
    rng = np.random.default_rng(14)
    img, pf, _ = build(la, "blur", 5, shape, rng, 0.75)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, bounds=(40, 200))
    x0 = img[None] + rng.normal(0, 10, (4,) + shape)
    outs = {}
    for variant in ("pipe", "pipe2", "auto"):
        smp = la.MYULASampler(pf, pg, shape, n_chains=4, tau=0.2 * 0.75 ** 2, gamma=0.75 ** 2, seed=5, variant=variant)
        smp.set_state(x0)
        smp.step(2)
        outs[variant] = smp.get_state().cpu().numpy()
        assert smp.kernel_name == ("myula_step_pipe_box_kernel" if variant == "pipe" else "myula_step_pipe_box2_kernel"), (variant, smp.kernel_name)
        smp.close()
    np.testing.assert_array_equal(outs["pipe"], outs["pipe2"])
    np.testing.assert_array_equal(outs["auto"], outs["pipe2"])
    free = la.MYULASampler(pf, la.TV(shape, sigma=TAU_REG, niter=10), shape, n_chains=4, tau=0.2 * 0.75 ** 2, gamma=0.75 ** 2, seed=5)
    free.set_state(x0)
    free.step(2)
    assert not np.array_equal(free.get_state().cpu().numpy(), outs["pipe"])      # the box did something
    free.close()


# ------------------------------------------------------------------ 5. separable priors
def separable(la, name, lo, hi):
    """(device prior, checker prior)"""
    b = (lo, hi)
    if name == "l1":
        return la.L1(sigma=0.8, bounds=b), Clipped(lambda x, t: O.L1(0.8).prox(x, t), lo, hi)
    if name == "l2":
        return la.L2(sigma=0.02, bounds=b), Clipped(lambda x, t: x / (1.0 + t * 0.02), lo, hi)
    if name == "laplace":
        return la.Laplace(0.6, bounds=b), Clipped(lambda x, t: O.prox_laplace(x, t * 0.6), lo, hi)
    if name == "huber":
        return la.Huber(2.0, 0.7, bounds=b), Clipped(lambda x, t: O.prox_huber(x, 2.0, t * 0.7), lo, hi)
    return la.Box(lo, hi), Clipped(lambda x, t: x, lo, hi)


SEPARABLE = ["l1", "l2", "laplace", "huber", "box"]


@pytest.mark.parametrize("name", SEPARABLE)
def test_separable_prox_is_the_clamped_prox(la, name):
    rng = np.random.default_rng(3)
    for lo, hi in [(40.0, 200.0), (-60.0, -10.0), (0.0, INF)]:
        pg, og = separable(la, name, lo, hi)
        for shape in [(33, 203), (7, 9), (1000,)]:
            x = rng.normal(60, 90, shape)
            for t in (0.5, 12.0):
                out = pg.prox(x, t)
                assert out.shape == x.shape
                e = rel(out, og.prox(x, t))
                assert e <= 1e-6, (name, lo, hi, shape, t, e)
                assert out.min() >= np.float32(lo) and out.max() <= np.float32(hi)


@pytest.mark.parametrize("name", SEPARABLE)
@pytest.mark.parametrize("data,shape", [("blur", (24, 96)), ("blur", (24, 264)), ("identity", (24, 264))])
def test_myula_steps_separable_box(la, name, data, shape):
    rng = np.random.default_rng(21)
    C_, nit, sigma = 3, 6, 6.0
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    img, pf, of = build(la, data, 5, shape, rng, sigma)
    pg, og = separable(la, name, 40.0, 200.0)
    x0 = img[None] + rng.normal(0, 10, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=gamma, noise="injected")
    smp.set_state(x0)
    ref = np.stack([O.myula(of, og, x0[c].ravel(), tau, gamma, niter=nit, noise=[noise[i, c].ravel() for i in range(nit)]).reshape((nit,) + shape)
                    for c in range(C_)], axis=1)
    for it in range(nit):
        smp.step(1, noise=noise[it:it + 1])
        e = rel(smp.get_state().cpu().numpy(), ref[it])
        print(f"{name} {data} {shape} step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    # without the box the same prior gives another trajectory: the clamp reached the step
    pg_free = {"l1": lambda: la.L1(sigma=0.8), "l2": lambda: la.L2(sigma=0.02), "laplace": lambda: la.Laplace(0.6), "huber": lambda: la.Huber(2.0, 0.7),
               "box": lambda: None}[name]()
    free = la.MYULASampler(pf, pg_free, shape, n_chains=C_, tau=tau, gamma=gamma, noise="injected")
    free.set_state(x0)
    free.step(nit, noise=noise)
    assert rel(free.get_state().cpu().numpy(), ref[-1]) > 1e-3
    free.close()
    smp.close()


def test_myula_steps_separable_box_with_per_pixel_epsg(la):
    """Array-valued epsg and a box: one launch forms clip(prox_{epsg[i] gamma g}(x))."""
    shape = (24, 264)
    rng = np.random.default_rng(22)
    C_, nit, sigma = 3, 6, 6.0
    gamma, tau = sigma ** 2, 0.2 * sigma ** 2
    img, pf, of = build(la, "blur", 5, shape, rng, sigma)
    pg, og = separable(la, "l1", 40.0, 200.0)
    eps = rng.uniform(0.5, 2.0, shape)
    x0 = img[None] + rng.normal(0, 10, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=gamma, epsg=eps, noise="injected")
    smp.set_state(x0)
    for it in range(nit):
        smp.step(1, noise=noise[it:it + 1])
    got = smp.get_state().cpu().numpy()
    ref = np.stack([O.myula(of, og, x0[c].ravel(), tau, gamma, epsg=eps.ravel(), niter=nit, noise=[noise[i, c].ravel() for i in range(nit)])[-1].reshape(shape)
                    for c in range(C_)])
    e = rel(got, ref)
    print(f"per-pixel epsg + box: rel {e:.3e} after {nit} steps ({smp.kernel_name})")
    assert e < STEP_TOL * nit, e
    smp.close()


# ------------------------------------------------------------------ 6. an infinite box, and no box
@pytest.mark.parametrize("shape,iso", [((24, 264), True), ((24, 96), True), ((24, 877), True), ((24, 264), False)])
def test_infinite_bounds_agree_with_no_bounds(la, shape, iso):
    x = prox_input(shape, 0.0)
    a = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=iso, bounds=(-INF, INF)).prox(x.ravel(), 50.0)
    b = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=iso, bounds=None).prox(x.ravel(), 50.0)
    assert rel(a, b) <= 1e-6, rel(a, b)
    a1 = la.L1(sigma=0.8, bounds=(-INF, INF)).prox(x, 3.0)
    assert rel(a1, la.L1(sigma=0.8).prox(x, 3.0)) <= 1e-6


@pytest.mark.parametrize("shape", [(40, 264), (40, 96)])
def test_no_bounds_is_the_default(la, shape):
    rng = np.random.default_rng(7)
    img, pf, _ = build(la, "blur", 5, shape, rng, 0.75)
    x0 = img[None] + rng.normal(0, 10, (3,) + shape)
    outs = []
    for pg in (la.TV(shape, sigma=TAU_REG, niter=10), la.TV(shape, sigma=TAU_REG, niter=10, isotropic=True, bounds=None)):
        smp = la.MYULASampler(pf, pg, shape, n_chains=3, tau=0.2 * 0.75 ** 2, gamma=0.75 ** 2, seed=2)
        smp.set_state(x0)
        smp.step(1)
        outs.append(smp.get_state().cpu().numpy())
        assert "box" not in smp.kernel_name
        smp.close()
    np.testing.assert_array_equal(outs[0], outs[1])


# ------------------------------------------------------------------ 7. refusals
def myula_config(la, prior, shape=(24, 264), data=None, **fields):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    prob = _Problem(shape, data, prior)
    for k, v in fields.items():
        setattr(prob.c, k, v)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = 2
    cfg.tau, cfg.gamma, cfg.epsg = 0.1, 0.5, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return prob, cfg


def last_error():
    from lmc_atomi_amd import _dev
    return _dev.lib().lmc_last_error().decode()


CREATE_REFUSALS = [
    ("tv", dict(box_lo=5.0, box_hi=5.0), LMC_E_INVALID), ("tv", dict(box_lo=7.0, box_hi=-7.0), LMC_E_INVALID),
    ("tv", dict(box_lo=float("nan")), LMC_E_INVALID), ("tv", dict(box_hi=float("nan")), LMC_E_INVALID), ("tv", dict(box_enable=2), LMC_E_INVALID),
    ("tv", dict(tv_niter=0), LMC_E_INVALID), ("tv_aniso", dict(tv_niter=0), LMC_E_INVALID),
    ("tv", dict(tv_rtol=1e-4), LMC_E_UNSUPPORTED), ("tv", dict(tv_warm=1), LMC_E_UNSUPPORTED), ("haar", dict(), LMC_E_UNSUPPORTED),
]


def prior_of(la, which, shape):
    from lmc_atomi_amd import _capi
    if which == "haar":
        return {"prior_kind": _capi.PRIOR_HAAR_L1, "prior_sigma": 0.3, "box": (40.0, 200.0)}
    return la.TV(shape, sigma=TAU_REG, niter=10, isotropic=which == "tv", bounds=(40, 200)).prior_descriptor()


@pytest.mark.parametrize("which,fields,status", CREATE_REFUSALS)
def test_c_abi_refuses_bad_bounds_and_what_is_not_built(la, which, fields, status):
    from lmc_atomi_amd import _dev
    shape = (24, 264)
    prob, cfg = myula_config(la, prior_of(la, which, shape), shape, **fields)
    assert prob.c.box_enable == 1 or "box_enable" in fields
    hnd = C.c_void_p()
    lib = _dev.lib()
    rc = lib.lmc_myula_create(C.byref(cfg), C.byref(hnd))
    msg = last_error()
    if rc == 0:
        lib.lmc_sampler_destroy(hnd)
    print(which, fields, "->", rc, msg)
    assert rc == status and msg, (rc, msg)
    # lmc_fused_eval refuses the same problem
    import torch
    x = torch.zeros(shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 1, 0.0, 0.0, 1.0, 1.0, _dev.stream_ptr(x.device))
    assert rc == status and last_error(), (rc, last_error())


def test_c_abi_samplers_without_a_box_form_refuse_it(la):
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    shape = (24, 264)
    prob, cfg = myula_config(la, prior_of(la, "tv", shape), shape)
    for create in (lambda h: lib.lmc_mymala_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_skrock_create(C.byref(cfg), 5, 0.05, C.byref(h))):
        hnd = C.c_void_p()
        rc = create(hnd)
        assert rc == LMC_E_UNSUPPORTED and "box" in last_error(), (rc, last_error())
        assert not hnd.value
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "box" in last_error(), (rc, last_error())
    # a MYULA handle with a box: its weight is fixed
    hnd = C.c_void_p()
    assert lib.lmc_myula_create(C.byref(cfg), C.byref(hnd)) == 0, last_error()
    rc = lib.lmc_sampler_set_prior_sigma(hnd, 0.5)
    assert rc == LMC_E_UNSUPPORTED and "box" in last_error(), (rc, last_error())
    sc = _capi.lmc_sapg_config()
    sc.struct_size = C.sizeof(_capi.lmc_sapg_config)
    sc.theta0, sc.theta_min, sc.theta_max, sc.dim_eff = 0.3, 1e-3, 1e2, 1000.0
    sc.step_scale, sc.step_exponent, sc.n_updates, sc.iters_per_update, sc.average_from = 10.0, 0.8, 2, 1, 0
    trace = (C.c_double * 3)()
    rc = lib.lmc_sampler_sapg(hnd, C.byref(sc), None, trace, None, None, None)
    assert rc == LMC_E_UNSUPPORTED and "box" in last_error(), (rc, last_error())
    lib.lmc_sampler_destroy(hnd)


@pytest.mark.parametrize("variant", [3, 4, 5, 6])
def test_c_abi_refuses_a_forced_variant_without_a_box_form(la, variant):
    """split, point, block and rows have no box form of the TV prior: the launch that would need one says so."""
    import torch
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    shape = (24, 264)
    prob, cfg = myula_config(la, prior_of(la, "tv", shape), shape, step_variant=variant)
    hnd = C.c_void_p()
    assert lib.lmc_myula_create(C.byref(cfg), C.byref(hnd)) == 0, last_error()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    assert lib.lmc_sampler_set_state(hnd, _dev.ptr(x), _dev.stream_ptr(x.device)) == 0
    rc = lib.lmc_sampler_step(hnd, 1, None, _dev.stream_ptr(x.device))
    torch.cuda.synchronize()
    msg = last_error()
    lib.lmc_sampler_destroy(hnd)
    assert rc == LMC_E_UNSUPPORTED and "box" in msg, (rc, msg)


def test_python_refusals(la):
    shape = (24, 264)
    for bad in [(5, 5), (7, -7), (float("nan"), 1), (0, float("nan")), (1,), "ab", 3.0]:
        for make in (lambda b: la.TV(shape, bounds=b), lambda b: la.L1(bounds=b), lambda b: la.L2(sigma=1.0, bounds=b), lambda b: la.Laplace(1.0, bounds=b)):
            with pytest.raises(ValueError):
                make(bad)
    with pytest.raises(ValueError):
        la.Box(3, 1)
    for iso in (True, False):
        with pytest.raises(NotImplementedError):
            la.TV(shape, niter=10, rtol=1e-4, isotropic=iso, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.TV(shape, niter=3, warm=True, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.WaveletL1(shape, sigma=0.3, bounds=(0, 255))
    with pytest.raises(NotImplementedError):
        la.L2(Op=la.Convolve2D(shape, np.ones((5, 5)) / 25, offset=(2, 2)), b=np.zeros(shape), bounds=(0, 255))
    rng = np.random.default_rng(0)
    img, pf, _ = build(la, "blur", 5, shape, rng, 0.75)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, bounds=(0, 255))
    kw = dict(n_chains=2, tau=0.1, gamma=0.5)
    with pytest.raises(NotImplementedError):
        la.MYMALASampler(pf, pg, shape, **kw)
    with pytest.raises(NotImplementedError):
        la.SKROCKSampler(pf, pg, shape, n_stages=5, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TAU_REG, niter=3, bounds=(0, 255)), shape, tv_warm=True, **kw)
    with pytest.raises(NotImplementedError):
        la.MoreauYosidaMetropolisAdjustedLangevin(pf, pg, img.ravel(), tau=0.1, gamma=0.5, niter=2, dims=shape)
    with pytest.raises(NotImplementedError):
        la.StabilisedLangevin(pf, pg, img.ravel(), tau=0.1, gamma=0.5, niter=2, n_stages=5, dims=shape)
    with pytest.raises(NotImplementedError):
        la.UnadjustedLangevinPrimalDual(pf, la.L1(sigma=0.3, bounds=(0, 255)), la.Gradient(shape), img.ravel(), tau=0.1, mu=0.1, niter=2)
    with pytest.raises(NotImplementedError):
        la.EstimatePriorWeight(pf, pg, img.ravel(), 0.1, 0.5, 4, (1e-3, 1e2), dims=shape)
    smp = la.MYULASampler(pf, pg, shape, **kw)
    with pytest.raises(NotImplementedError):
        smp.set_prior_weight(0.5)
    with pytest.raises(NotImplementedError):
        smp.estimate_prior_weight(4, (1e-3, 1e2))
    smp.close()


def test_functional_interface_and_diagnostics_take_a_box(la):
    """`MoreauYosidaUnadjustedLangevin` with the moment, histogram and group-moment keywords runs a box-constrained prior."""
    shape = (24, 264)
    rng = np.random.default_rng(1)
    img, pf, _ = build(la, "blur", 5, shape, rng, 6.0)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, bounds=(40, 200))
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, img.ravel(), tau=7.2, gamma=36.0, niter=8, seed=3, n_chains=4, dims=shape, moment_scales=(2,),
                                            hist_bins=8, hist_range=(0.0, 255.0), chain_groups=2)
    assert res.count > 0 and np.isfinite(np.asarray(res.mean.cpu() if hasattr(res.mean, "cpu") else res.mean)).all()
