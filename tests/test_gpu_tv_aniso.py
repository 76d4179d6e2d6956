"""GPU parity of the anisotropic TV prior, g(x) = sigma (||d_r x||_1 + ||d_c x||_1), as `TV(..., isotropic=False)`: the prox alone, inside the
fused MYULA step (pipe kernel `myula_step_pipe_aniso_kernel` and the tile fallback), in MYMALA, and the refusals of the C ABI.

The reference of the prox is `tv_prox_aniso` (tests/_tv_aniso_ref.py): the checker's `tv_prox_fgp` (oracle/lmc_oracle.py) with the projection of the dual onto the
l-infinity unit ball (`np.clip`) instead of the pixel-norm ball -- the set `L1.proxdual` projects onto.  Everything else (blur, gradients, momentum
tables, the MC-TV term) is the checker's own.

Tolerances are the project's (tests/test_gpu_parity.py): one operator / one step rel-L2 <= 1e-5, and 1e-5 x (step index) along a trajectory.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import lmc_oracle as O
from tests._tv_aniso_ref import tv_aniso_value, tv_prox_aniso

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
SIGMA, TAU_REG = 0.75, 0.3
GAMMA, TAU = SIGMA ** 2, 0.2 * SIGMA ** 2


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


class AnisoTV:
    """The checker-side prior object (what O.myula calls)."""

    def __init__(self, dims, sigma, niter):
        self.dims, self.sigma, self.niter = dims, sigma, niter

    def prox(self, x, t):
        return tv_prox_aniso(np.asarray(x).reshape(self.dims), self.sigma * t, self.niter).ravel()


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


# ------------------------------------------------------------------ 1. the prox alone
PROX_CASES = [(10, (16, 16), 0.16875, False), (10, (100, 70), 0.16875, False), (10, (40, 264), 0.16875, False), (10, (24, 877), 0.16875, False),
              (20, (64, 136), 2.0, False), (10, (65, 129), 15.0, False), (50, (40, 200), 1.0, False), (6, (33, 520), 0.5, False),
              (1, (8, 8), 2.0, False), (9, (40, 96), 0.5, False), (9, (40, 96), 0.5, True)]


@pytest.mark.parametrize("niter,shape,gamma,lagged", PROX_CASES)
def test_aniso_prox_matches_reference(la, niter, shape, gamma, lagged):
    rng = np.random.default_rng(niter)
    img, _, _ = synth(*shape, seed=1)
    x = img + rng.normal(0, 8, shape)
    for momentum in ("unlocbox", "fista"):
        # lagged_output: niter = 10 asked for, the iterate after 9 dual updates returned (with the first 9 entries of the 10-entry momentum table)
        tv = la.TV(shape, sigma=0.3, niter=niter + 1 if lagged else niter, momentum=momentum, lagged_output=lagged, isotropic=False)
        ref = tv_prox_aniso(x, gamma, niter, momentum=momentum)         # prox parameter tau = gamma / 0.3, sigma = 0.3
        out = tv.prox(x.ravel(), gamma / 0.3)
        assert out.shape == (shape[0] * shape[1],)
        e = rel(out, ref.ravel())
        print(f"prox niter={niter} shape={shape} gamma={gamma} {momentum}: rel {e:.3e}; vs isotropic {rel(O.tv_prox_fgp(x, gamma, niter, momentum=momentum), ref):.2e}")
        assert e < STEP_TOL, (momentum, e)
    val, vref = tv(x.ravel()), 0.3 * float(tv_aniso_value(x))
    print(f"value: {val:.8e} vs {vref:.8e}")
    assert abs(val - vref) <= 1e-5 * vref


def test_aniso_prox_batch(la):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(6, 30, 264)) * 30
    out = la.TV((30, 264), sigma=1.0, niter=10, isotropic=False).prox(x, 0.7)
    assert out.shape == x.shape
    assert rel(out, tv_prox_aniso(x, 0.7, 10)) < STEP_TOL


# ------------------------------------------------------------------ 2. fused MYULA step, injected noise
def build(la, data, k, shape, rng, ncvx=False):
    """(device data term, checker data term, x0 base image)"""
    img, h, y = synth(*shape, seed=2, k=max(k, 3))
    n = shape[0] * shape[1]
    if data == "blur":
        off = (k // 2, k // 2)
        Op, oOp = la.Convolve2D(shape, h, offset=off), O.Convolve2D(shape, h, off)
    elif data == "identity":
        y = img + rng.normal(0, SIGMA, shape)
        Op, oOp = None, None
    else:
        mask = (rng.uniform(size=shape) < 0.5).astype(np.float64)
        y = mask * img + rng.normal(0, SIGMA, shape) * mask
        Op, oOp = la.Diagonal(mask, dims=shape), O.Diagonal(mask)
    if ncvx:
        kw = dict(dims=shape, b=y.ravel(), sigma=1 / SIGMA ** 2, lamda=0.3, gamma=15.0, isotropic=True, niter=20)
        return img, la.L2_ncvx_tv(Op=Op, Op2=la.Gradient(shape), **kw), O.L2NcvxTV(Op=oOp, Op2=O.Gradient(shape), **kw)
    return img, la.L2(Op=Op, b=y.ravel(), sigma=1 / SIGMA ** 2, dims=shape), O.L2(Op=oOp, b=y.ravel(), sigma=1 / SIGMA ** 2)


def pipe_covers(W, niter):
    return W > 128 and niter % 10 == 0 and 10 <= niter <= 60


STEP_CASES = [("blur", 5, (32, 96), 10), ("blur", 5, (24, 136), 10), ("blur", 6, (28, 200), 10), ("blur", 7, (30, 203), 10), ("blur", 5, (40, 264), 10),
              ("blur", 7, (24, 512), 10), ("blur", 6, (33, 333), 10), ("blur", 5, (24, 877), 10), ("blur", 7, (24, 1100), 10),
              ("identity", 0, (32, 200), 10), ("identity", 0, (24, 333), 10), ("identity", 0, (24, 96), 10), ("identity", 0, (24, 877), 10),
              ("mask", 0, (33, 264), 10), ("mask", 0, (25, 203), 10), ("mask", 0, (24, 1100), 10), ("blur", 5, (24, 203), 10), ("blur", 5, (24, 512), 10),
              ("blur", 5, (40, 264), 7), ("blur", 5, (24, 264), 50), ("blur", 5, (24, 877), 50), ("blur", 5, (32, 264), 20), ("mc", 5, (32, 264), 10)]


@pytest.mark.parametrize("data,k,shape,niter", STEP_CASES)
def test_myula_steps_aniso_injected_noise(la, data, k, shape, niter):
    rng = np.random.default_rng(11)
    C_, nit = 3, 4
    img, pf, of = build(la, "blur" if data == "mc" else data, k, shape, rng, ncvx=data == "mc")
    pg, og = la.TV(shape, sigma=TAU_REG, niter=niter, isotropic=False), AnisoTV(shape, TAU_REG, niter)
    x0 = img[None] + rng.normal(0, 10, (C_,) + shape)
    noise = rng.standard_normal((nit, C_) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=TAU, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    ref = np.stack([O.myula(of, og, x0[c].ravel(), TAU, GAMMA, niter=nit, noise=[noise[i, c].ravel() for i in range(nit)]).reshape((nit,) + shape)
                    for c in range(C_)], axis=1)        # [nit, C, H, W]
    for it in range(nit):
        smp.step(1, noise=noise[it:it + 1])
        got = smp.get_state().cpu().numpy()
        e = rel(got, ref[it])
        print(f"{data} k={k} {shape} niter={niter} step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
        if shape[1] > 512:            # column-wise: nothing special at the strip seams or in the last columns (tests/test_gpu_wide.py)
            colerr = np.abs(got - ref[it]).max(axis=(0, 1))
            assert colerr.max() < 2e-3, (int(colerr.argmax()), float(colerr.max()))
    assert ("pipe_aniso" if pipe_covers(shape[1], niter) else "tile") in smp.kernel_name, smp.kernel_name
    assert smp.iteration == nit
    smp.close()


# ------------------------------------------------------------------ 3. kernel variants agree
@pytest.mark.parametrize("shape,K", [((64, 264), 10), ((40, 520), 10), ((40, 264), 20)])
def test_tile_and_auto_variants_agree(la, shape, K):
    rng = np.random.default_rng(13)
    img, pf, _ = build(la, "blur", 5, shape, rng)
    pg = la.TV(shape, sigma=TAU_REG, niter=K, isotropic=False)
    x0 = img[None] + rng.normal(0, 10, (4,) + shape)
    outs, names = {}, {}
    for variant in ("tile", "auto"):
        smp = la.MYULASampler(pf, pg, shape, n_chains=4, tau=TAU, gamma=GAMMA, seed=5, variant=variant)
        smp.set_state(x0)
        smp.step(1)
        outs[variant], names[variant] = smp.get_state().cpu().numpy(), smp.kernel_name
        smp.close()
    assert "tile" in names["tile"] and "pipe_aniso" in names["auto"], names
    e = rel(outs["auto"], outs["tile"])
    print(f"{shape} K={K}: tile vs auto rel {e:.3e}")
    assert e <= 2e-6, e


@pytest.mark.parametrize("shape", [(64, 264), (40, 512)])
def test_one_team_and_two_team_layouts_are_bit_identical(la, shape):
    """Every pixel runs the one-team kernel's arithmetic on the same operands (as for the isotropic prior); auto picks the two-team layout here."""
    rng = np.random.default_rng(14)
    img, pf, _ = build(la, "blur", 5, shape, rng)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False)
    x0 = img[None] + rng.normal(0, 10, (4,) + shape)
    outs = {}
    for variant in ("pipe", "pipe2", "auto"):
        smp = la.MYULASampler(pf, pg, shape, n_chains=4, tau=TAU, gamma=GAMMA, seed=5, variant=variant)
        smp.set_state(x0)
        smp.step(2)
        outs[variant] = smp.get_state().cpu().numpy()
        assert "pipe_aniso" in smp.kernel_name
        smp.close()
    np.testing.assert_array_equal(outs["pipe"], outs["pipe2"])
    np.testing.assert_array_equal(outs["auto"], outs["pipe2"])


def test_two_team_layout_refuses_what_it_does_not_cover(la):
    shape = (24, 203)
    rng = np.random.default_rng(15)
    img, pf, _ = build(la, "blur", 5, shape, rng)
    smp = la.MYULASampler(pf, la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False), shape, n_chains=2, tau=TAU, gamma=GAMMA, variant="pipe2")
    smp.set_state(img)
    with pytest.raises(la.LMCError) as ei:
        smp.step(1)
    assert ei.value.code == LMC_E_UNSUPPORTED
    smp.close()


# ------------------------------------------------------------------ 4. sampler behaviour
@pytest.mark.parametrize("shape", [(24, 264), (24, 96)])
def test_multi_step_call_equals_single_steps_and_is_reproducible(la, shape):
    rng = np.random.default_rng(4)
    img, pf, _ = build(la, "blur", 5, shape, rng)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False)
    mk = lambda: la.MYULASampler(pf, pg, shape, n_chains=4, tau=TAU, gamma=GAMMA, seed=9)
    a, b, c = mk(), mk(), mk()
    for s in (a, b, c):
        s.set_state(img)
    a.step(6)
    for _ in range(6):
        b.step(1)
    c.step(6)
    xa, xb, xc = (s.get_state().cpu().numpy() for s in (a, b, c))
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(xa, xc)
    assert not np.array_equal(xa[0], xa[1])
    for s in (a, b, c):
        s.close()


# ------------------------------------------------------------------ 5. MYMALA
@pytest.mark.parametrize("shape", [(32, 32), (20, 264)])
def test_mymala_one_iteration_log_alpha(la, shape):
    rng = np.random.default_rng(17)
    img = np.zeros(shape)
    img[shape[0] // 4:shape[0] // 2, shape[1] // 4:3 * shape[1] // 4] = 150.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h, off = np.ones((5, 5)) / 25, (2, 2)
    y = O.blur(img, h, off) + rng.normal(0, SIGMA, shape)
    sf = 1 / SIGMA ** 2
    tau = 0.02 * SIGMA ** 2
    C_, seed, off_c = 6, 1234, 40
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=sf)
    pg = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False)
    x0 = img[None] + rng.normal(0, 3, (C_,) + shape)
    noise = rng.standard_normal((1, C_) + shape)
    smp = la.MYMALASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=GAMMA, noise="injected", seed=seed, chain_offset=off_c)
    smp.set_state(x0)
    smp.step(1, noise=noise)
    acc_d, la_d = smp.acceptance()
    acc_d, la_d = acc_d.cpu().numpy(), la_d.cpu().numpy()
    got = smp.get_state().cpu().numpy()
    name = smp.kernel_name
    smp.close()

    # float64, formed here: proposal mean m(v), potential U(v) = f(v) + g(v), log alpha = U(x) - U(x') - (||x - m(x')||^2 - ||x' - m(x)||^2) / (4 tau)
    def mean(v):
        g = sf * O.blur_adjoint(O.blur(v, h, off) - y, h, off)
        return (1 - tau / GAMMA) * v - tau * g + tau / GAMMA * tv_prox_aniso(v, TAU_REG * GAMMA, 10)

    def U(v):
        r = O.blur(v, h, off) - y
        return 0.5 * sf * np.sum(r * r, axis=(-2, -1)) + TAU_REG * tv_aniso_value(v)

    mx = mean(x0)
    xp = mx + np.sqrt(2 * tau) * noise[0]
    mxp = mean(xp)
    la_o = (U(x0) - U(xp)) - (np.sum((x0 - mxp) ** 2, axis=(-2, -1)) - np.sum((xp - mx) ** 2, axis=(-2, -1))) / (4 * tau)
    scale = np.abs(U(x0)).max()
    bound = 2e-6 * scale + 2e-3
    err = np.abs(la_d - la_o)
    print(f"{shape} ({name}): log alpha device {la_d} checker {la_o}; max err {err.max():.3e}, bound {bound:.3e}")
    assert (err < bound).all(), (err.max(), bound)
    us = O.philox_uniforms(seed, 0, off_c + np.arange(C_))
    safe = np.abs(np.log(us) - la_o) > 10 * bound
    assert safe.sum() >= C_ // 2, "test problem too borderline"
    ok = np.log(us) <= la_o
    want = np.where(ok[:, None, None], xp, x0)
    assert (acc_d[safe] == ok[safe]).all(), (acc_d, ok)
    assert rel(got[safe], want[safe]) < 2e-5
    assert ("pipe_aniso" if shape[1] > 128 else "tile") in name, name


# ------------------------------------------------------------------ 6. refusals of the C ABI


@pytest.mark.parametrize("field,value,status", [("tv_niter", 0, LMC_E_INVALID), ("tv_rtol", 1e-4, LMC_E_UNSUPPORTED), ("tv_warm", 1, LMC_E_UNSUPPORTED),
                                                ("step_variant", 3, LMC_E_UNSUPPORTED)])
def test_c_abi_refuses_what_is_not_built(la, field, value, status):
    import torch
    from lmc_atomi_amd import _capi, _dev
    from lmc_atomi_amd.proximal import _Problem
    shape = (24, 264)
    rng = np.random.default_rng(3)
    _, pf, _ = build(la, "blur", 5, shape, rng)
    prob = _Problem(shape, pf.descriptor(), la.TV(shape, sigma=TAU_REG, niter=10, isotropic=False).prior_descriptor())
    assert prob.c.prior_kind == _capi.PRIOR_TV_ANISO and prob.c.tv_niter == 10
    setattr(prob.c, field, value)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = 2
    cfg.tau, cfg.gamma, cfg.epsg = TAU, GAMMA, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    hnd = C.c_void_p()
    lib = _dev.lib()
    rc = lib.lmc_myula_create(C.byref(cfg), C.byref(hnd))
    if rc == 0:                       # a forced kernel variant is refused by the launch that would need it
        x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
        assert lib.lmc_sampler_set_state(hnd, _dev.ptr(x), _dev.stream_ptr(x.device)) == 0
        rc = lib.lmc_sampler_step(hnd, 1, None, _dev.stream_ptr(x.device))
        torch.cuda.synchronize()
        lib.lmc_sampler_destroy(hnd)
    msg = lib.lmc_last_error().decode()
    print(field, value, "->", rc, msg)
    assert rc == status, (rc, msg)
    assert msg


def test_fused_eval_refuses_a_prox_without_iterations(la):
    from lmc_atomi_amd.proximal import _Problem
    shape = (16, 40)
    prob = _Problem(shape, prior={"prior_kind": 4, "prior_sigma": 0.3})      # LMC_PRIOR_TV_ANISO as ULPDA passes it: no tv_niter
    x = np.random.default_rng(0).normal(size=shape)
    with pytest.raises(la.LMCError) as ei:
        prob.eval(x, 0.0, 0.0, 1.0, 0.5)
    assert ei.value.code == LMC_E_INVALID
    f, g = prob.energies(x)          # ... which the energies still accept
    assert abs(float(g[0]) - 0.3 * float(tv_aniso_value(x))) <= 1e-5 * float(g[0])


# ------------------------------------------------------------------ 7. the isotropic prior did not move
@pytest.mark.parametrize("shape", [(40, 264), (40, 96)])
def test_isotropic_argument_is_the_default(la, shape):
    rng = np.random.default_rng(7)
    img, pf, _ = build(la, "blur", 5, shape, rng)
    x0 = img[None] + rng.normal(0, 10, (3,) + shape)
    outs = []
    for pg in (la.TV(shape, sigma=TAU_REG, niter=10), la.TV(shape, sigma=TAU_REG, niter=10, isotropic=True)):
        smp = la.MYULASampler(pf, pg, shape, n_chains=3, tau=TAU, gamma=GAMMA, seed=2)
        smp.set_state(x0)
        smp.step(1)
        outs.append(smp.get_state().cpu().numpy())
        assert "aniso" not in smp.kernel_name
        smp.close()
    np.testing.assert_array_equal(outs[0], outs[1])
