"""Every entry point with more images than one grid dimension holds (65535): the stateless operators on 2 * 65535 + 7 = 131077 images, the samplers
with 65535 + 8 = 65543 chains.  Nothing else in the suite runs a kernel with more than a few thousand images, while the library has a dozen
branches that exist only beyond that: launchers that split the image axis into chunks of 65535 and advance every pointer by the chunk start, fused
kernels that put the images on gridDim.x and hold `blocks per image * images` in an int, moment reductions that cut the chains into segments, and
the 32-bit Philox counter word of the global chain id.

The batches are 7 patterns tiled (tests/_many.py): the checker runs on the 7 patterns, the expectation for image c is ref[c % 7], and because
65535 % 7 == 1 a chunk whose pointer lost its offset holds the wrong pattern.  Errors are per image, against the project's tolerances: 1e-5 for one
operator / one step, 5e-6 x steps for a short trajectory, 1e-9 for moments against fp64 sums.  Every sampler case asserts the kernel that ran.

Found by these tests and fixed with them: the 1-D TV launchers of the anisotropic ME-TV term (launch_tv1d_sol / _iter / _objective) returned
hipErrorInvalidConfiguration above 65535 images -- LMC_E_HIP "invalid configuration" from the middle of a step; they now loop over chunks of 65535
like their neighbours (test_me_tv_aniso_term_past_65535_images)."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
from tests import _many as M

pytestmark = pytest.mark.gpu

N, C, P = M.N_OPS, M.C_SMP, M.P
STEP_TOL, SIGMA, TAU_REG, GAMMA, TAU = M.STEP_TOL, M.SIGMA, M.TAU_REG, M.GAMMA, M.TAU
SF = 1 / SIGMA ** 2
NOISE_TOL = 2e-5           # Philox field against the checker, max abs: hardware log2 / sqrt / sin / cos (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free_hbm():
    yield
    import torch
    torch.cuda.empty_cache()


def problem(la, shape, data=None, prior=None):
    from lmc_atomi_amd.proximal import _Problem
    return _Problem(shape, data=data, prior=prior)


# =========================================================================================== stateless entry points, 131077 images
def test_blur_and_adjoint_past_two_chunks(la):
    """z-chunks of launch_blur: 5 x 7 images, 3 x 3 kernel whose origin is its top right tap"""
    shape, off = (5, 7), (0, 2)
    x7 = M.patterns(shape, 1)
    X = M.tile_dev(x7, N).reshape(N, -1)
    Op = la.Convolve2D(shape, M.H3_NONSEP, offset=off)
    M.check_per_image(Op.matvec(X), O.blur(x7, M.H3_NONSEP, off), STEP_TOL, "Convolve2D.matvec")
    M.check_per_image(Op.rmatvec(X), O.blur_adjoint(x7, M.H3_NONSEP, off), STEP_TOL, "Convolve2D.rmatvec")


def test_gradient_and_dual_projections_past_two_chunks(la):
    """grid-stride loops over img * n_img: Gradient.matvec / rmatvec, L21.proxdual, L1.proxdual"""
    shape = (5, 7)
    n = shape[0] * shape[1]
    x7 = M.patterns(shape, 2)
    v7 = np.random.default_rng(3).normal(0, 0.4, (P, 2 * n))            # a dual field: entries on both sides of the ball of radius 0.3
    G, Go = la.Gradient(shape), O.Gradient(shape)
    X, V = M.tile_dev(x7, N).reshape(N, -1), M.tile_dev(v7, N)
    M.check_per_image(G.matvec(X), np.stack([Go.matvec(x.ravel()) for x in x7]), STEP_TOL, "Gradient.matvec")
    M.check_per_image(G.rmatvec(V), np.stack([Go.rmatvec(v) for v in v7]), STEP_TOL, "Gradient.rmatvec")
    M.check_per_image(la.L21(sigma=0.3).proxdual(V, 1.0), np.stack([O.L21(sigma=0.3).proxdual(v, 1.0) for v in v7]), STEP_TOL, "L21.proxdual")
    M.check_per_image(la.L1(sigma=0.3).proxdual(V, 1.0), np.clip(v7, -0.3, 0.3), STEP_TOL, "L1.proxdual")
    M.check_per_image(la.L1(sigma=0.3).prox(X, 20.0), O.L1(sigma=0.3).prox(x7.reshape(P, -1), 20.0), STEP_TOL, "L1.prox (lmc_prox_elementwise)")


def test_haar_prox_and_value_past_two_chunks(la):
    """chunked y of both Haar kernels (out + z0, val + z0), 8 x 8"""
    shape = (8, 8)
    x7 = M.patterns(shape, 4)
    X = M.tile_dev(x7, N)
    w = la.WaveletL1(shape, sigma=2.0)
    M.check_per_image(w.prox(X, 0.7), O.haar_l1_prox(x7, 1.4), STEP_TOL, "lmc_haar_l1_prox")
    M.check_per_image(w(X), 2.0 * O.haar_l1_value(x7), STEP_TOL, "Haar g")


def test_energies_every_data_kind_and_prior_past_two_chunks(la):
    """energy_kernel over chunks of 65535 (x + z0 img, f_out + z0, g_out + z0): no / identity / mask / non-separable blur data terms, priors
    L2, L1, TV_ISO, TV_ANISO"""
    shape = (5, 7)
    x7 = M.patterns(shape, 5)
    X = M.tile_dev(x7, N)
    rng = np.random.default_rng(6)
    y = x7[3] + rng.normal(0, SIGMA, shape)
    mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    h, off = M.H3_NONSEP, (1, 1)
    yb = O.blur(x7[3], h, off) + rng.normal(0, SIGMA, shape)
    datas = {"none": (None, (None, None, None)),
             "identity": (la.L2(b=y, sigma=SF, dims=shape), (y, None, None)),
             "mask": (la.L2(Op=la.Diagonal(mask, dims=shape), b=mask * y, sigma=SF, dims=shape), (mask * y, None, mask)),
             "blur": (la.L2(Op=la.Convolve2D(shape, h, offset=off), b=yb, sigma=SF), (yb, h, None))}
    priors = {"l2": (la.L2(sigma=0.05), {"kind": "l2", "sigma": 0.05}), "l1": (la.L1(sigma=0.4), {"kind": "l1", "sigma": 0.4}),
              "tv": (la.TV(shape, sigma=TAU_REG), {"kind": "tv", "sigma": TAU_REG}), "tv_aniso": (la.TV(shape, sigma=TAU_REG, isotropic=False), None)}
    for dn, (pf, (yy, hh, mm)) in datas.items():
        for pn, (pg, op) in priors.items():
            f, g = problem(la, shape, pf.descriptor() if pf else None, pg.prior_descriptor()).energies(X)
            if pf is None:
                fo = np.zeros(P)
            else:
                fo, _ = O.energies(x7, yy, hh, off, SF, {"kind": "none"}, mask=mm)
            go = TAU_REG * M.tv_aniso_value(x7) if op is None else O.energies(x7, x7[0], None, None, 1.0, op)[1]
            M.check_per_image(f, fo, STEP_TOL, f"lmc_energies f, data {dn}, prior {pn}")
            M.check_per_image(g, go, STEP_TOL, f"lmc_energies g, data {dn}, prior {pn}")


def test_energies_separable_blur_past_two_chunks(la):
    """energy_sep_kernel: tiles * n_img workgroups on gridDim.x, 5 x 5 box on 6 x 10"""
    shape = (6, 10)
    x7 = M.patterns(shape, 7)
    h, off, y = M.blur_problem(shape, 5)
    pf, pg = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=SF), la.TV(shape, sigma=TAU_REG)
    f, g = problem(la, shape, pf.descriptor(), pg.prior_descriptor()).energies(M.tile_dev(x7, N))
    fo, go = O.energies(x7, y, h, off, SF, {"kind": "tv", "sigma": TAU_REG})
    M.check_per_image(f, fo, STEP_TOL, "lmc_energies f, separable blur")
    M.check_per_image(g, go, STEP_TOL, "lmc_energies g, separable blur")


@pytest.mark.parametrize("term", ["mc_tv", "me_tv", "me_tv_aniso"])
def test_energies_with_the_non_convex_terms_past_two_chunks(la, term):
    """f(x) = sigma/2 ||M x - b||^2 - lamda env_gamma(.): the MC-TV envelope inside the energy kernel, the ME-TV one through the inner prox,
    sqdiff_kernel and axpy_env (isotropic: 2-D TV; anisotropic: the 1-D TV of the flattened image, launch_tv1d_*)"""
    shape = (4, 6)
    x7 = M.patterns(shape, 8)
    rng = np.random.default_rng(9)
    mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    b = (mask * (x7[2] + rng.normal(0, SIGMA, shape))).ravel()
    kw = dict(dims=shape, b=b, sigma=SF, lamda=0.3, gamma=15.0 if term != "mc_tv" else 2.0, isotropic=term != "me_tv_aniso", niter=10)
    pf = la.L2_ncvx_tv(Op=la.Diagonal(mask, dims=shape), Op2=la.Gradient(shape) if term == "mc_tv" else None, rtol=0.0, **kw)
    of = O.L2NcvxTV(Op=O.Diagonal(mask.ravel()), Op2=O.Gradient(shape) if term == "mc_tv" else None, **kw)
    f = pf(M.tile_dev(x7, N))
    M.check_per_image(f, np.array([of(x.ravel()) for x in x7]), STEP_TOL, f"lmc_energies f with the {term} term")


@pytest.mark.parametrize("shape,iso", [((6, 10), True), ((6, 10), False), ((2, 136), True), ((2, 136), False)])
def test_tv_prox_past_two_chunks(la, shape, iso):
    """TV.prox, fixed count: W <= 128 the tile / split kernels with tiles * C workgroups, W > 128 the full-width pipeline"""
    x7 = M.patterns(shape, 10)
    out = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=iso).prox(M.tile_dev(x7, N), GAMMA)
    ref = O.tv_prox_fgp(x7, TAU_REG * GAMMA, 10) if iso else M.tv_prox_aniso(x7, TAU_REG * GAMMA, 10)
    M.check_per_image(out, ref, STEP_TOL, f"TV.prox {shape} isotropic={iso}")


def test_tv_prox_early_exit_pass_by_pass_past_two_chunks(la):
    """rtol = 1e-4 on 6 x 10: tv_objective, tv_rtol_decide and tv_rtol_select with the images on gridDim.x.  The patterns leave in passes
    10, 4 and 2 (tests/test_many_images_reference.py), and an iterate of another pass misses the tolerance by a factor of ten and more."""
    shape = (6, 10)
    x7 = M.rtol_patterns(shape)
    ref, passes = M.rtol_reference(x7)
    assert len(set(passes.tolist())) >= 3, passes
    tv = la.TV(shape, sigma=M.RTOL_GAM / GAMMA, niter=M.RTOL_K, rtol=M.RTOL, exit_path="passes")
    M.check_per_image(tv.prox(M.tile_dev(x7, N), GAMMA), ref, STEP_TOL, f"TV.prox rtol, pass by pass (passes {passes.tolist()})")


def test_tv_prox_early_exit_on_the_device_past_two_chunks(la):
    """rtol = 1e-4 on 2 x 136: tv_rt_begin / tv_rt_decide over the chains and the per-chain counts inside the pipeline; the stateless prox on
    131077 images, and through a sampler (65543 chains) the pass every chain left in"""
    shape = (2, 136)
    x7 = M.rtol_patterns(shape)
    ref, passes = M.rtol_reference(x7)
    assert len(set(passes.tolist())) >= 3, passes
    tv = la.TV(shape, sigma=M.RTOL_GAM / GAMMA, niter=M.RTOL_K, rtol=M.RTOL)
    M.check_per_image(tv.prox(M.tile_dev(x7, N), GAMMA), ref, STEP_TOL, f"TV.prox rtol, device path (passes {passes.tolist()})")
    smp = la.MYULASampler(None, tv, shape, n_chains=C, tau=TAU, gamma=GAMMA, noise="none")
    smp.set_state(M.tile_dev(x7, C))
    smp.step(1)
    assert "per-chain exit" in smp.kernel_name, smp.kernel_name
    ps, reruns = smp.tv_exit_stats("prior")
    ps = ps.cpu().numpy()
    bad = np.flatnonzero(ps != M.tile(passes, C))
    assert bad.size == 0, f"{bad.size} chains left in another pass than the checker's, first: chain {bad[0]} (index {bad[0] % M.CHUNK}): {ps[bad[0]]} vs {passes[bad[0] % P]}"
    assert reruns[3] == 0
    M.check_per_image(smp.get_state(), (1 - TAU / GAMMA) * x7 + (TAU / GAMMA) * ref, STEP_TOL, "prox-only MYULA step with the device-side exit")
    smp.close()


@pytest.mark.parametrize("path", ["cg", "chebyshev"])
def test_l2_implicit_step_past_two_chunks(la, path):
    """L2.prox = (I + tau sigma H^T H)^-1 (x + tau sigma H^T b): CG for a non-separable 3 x 3 kernel, Chebyshev for the separable 5 x 5 box -- the
    per-chain stopping tests (cg_check, cheb_count) run over all images.  Both solvers stop at a relative residual; it is set to 1e-7 here so that
    the solve is converged well below the 1e-5 this test asks for (the default 1e-6 leaves up to 2e-5, tests/test_gpu_ulpda.py)."""
    shape = (5, 7) if path == "cg" else (4, 8)
    x7 = M.patterns(shape, 11)
    if path == "cg":
        h, off = M.H3_NONSEP, (1, 1)
        y = O.blur(x7[1], h, off)
    else:
        h, off, y = M.blur_problem(shape, 5)
    prev = la.set_cg_tolerance(1e-7)
    try:
        out = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y.ravel(), sigma=SF, niter=50, warm=False).prox(M.tile_dev(x7, N).reshape(N, -1), 0.53)
    finally:
        la.set_cg_tolerance(prev)
    l2o = O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=SF, niter=60, warm=False)
    M.check_per_image(out, np.stack([l2o.prox(x.ravel(), 0.53) for x in x7]), STEP_TOL, f"L2.prox ({path})")


# =========================================================================================== MYULA, 65543 chains, every kernel family
def blur_terms(la, shape, h, off, y):
    return la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=SF), (y, h, off, None)


def mask_terms(la, shape, seed=12):
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    y = mask * (M.patterns(shape, seed, noise=0.0)[3] + rng.normal(0, SIGMA, shape))
    return la.L2(Op=la.Diagonal(mask, dims=shape), b=y, sigma=SF, dims=shape), (y, None, None, mask)


def tv_prior(la, shape, niter=10, iso=True, **kw):
    return la.TV(shape, sigma=TAU_REG, niter=niter, isotropic=iso, **kw), {"kind": "tv" if iso else "tv_aniso", "sigma": TAU_REG, "niter": niter, "t": GAMMA}


def family(la, name):
    """(shape, device data term, checker data term (y, h, off, mask), device prior, checker prior, sampler arguments, kernel name, steps)"""
    box = lambda shape: blur_terms(la, shape, *M.blur_problem(shape, 5))
    if name in ("tile", "tile_aniso"):
        shape = (6, 10)
        return (shape, *box(shape), *tv_prior(la, shape, iso=name == "tile"), dict(variant="tile"), "myula_step_tile_kernel", 1)
    if name == "split":
        shape = (6, 10)
        return (shape, *box(shape), *tv_prior(la, shape), dict(variant="split"), "myula_step_split_kernel", 1)
    if name == "point":              # closed-form prior, no stencil: identity data term + l1
        shape = (5, 7)
        y = M.patterns(shape, 13)[2]
        return (shape, la.L2(b=y, sigma=SF, dims=shape), (y, None, None, None), la.L1(sigma=0.4), {"kind": "l1", "sigma": 0.4, "t": GAMMA}, dict(variant="point"),
                "myula_step_point_kernel", 1)
    if name in ("block", "block_mc_tv"):
        shape = (8, 8)
        pf, dat = mask_terms(la, shape)
        return (shape, pf, dat, la.WaveletL1(shape, sigma=TAU_REG), {"kind": "haar", "sigma": TAU_REG, "t": GAMMA}, dict(policy={"iterations_per_launch": 1}),
                "myula_step_block_kernel", 2)
    if name == "rows":               # separable blur + l1: barrier-free row streaming
        shape = (3, 8)
        return (shape, *box(shape), la.L1(sigma=0.4), {"kind": "l1", "sigma": 0.4, "t": GAMMA}, dict(policy={"iterations_per_launch": 1}), "myula_step_rows_kernel", 2)
    if name in ("pipe", "pipe_aniso"):
        shape = (2, 136)
        return (shape, *box(shape), *tv_prior(la, shape, iso=name == "pipe"), dict(variant="pipe"),
                "myula_step_pipe_kernel" if name == "pipe" else "myula_step_pipe_aniso_kernel", 1)
    if name == "pipe2":
        shape = (2, 264)
        return (shape, *box(shape), *tv_prior(la, shape), dict(variant="pipe2"), "myula_step_pipe_kernel", 1)
    if name == "pipe_chained":       # 20 dual iterations: two launches of 10 that hand the dual state over in HBM
        shape = (1, 136)
        return (shape, *box(shape), *tv_prior(la, shape, niter=20), {}, "myula_step_pipe_kernel", 1)
    if name == "pipe_warm":          # 3 dual iterations per step from the dual of the previous step
        shape = (2, 136)
        pg, op = tv_prior(la, shape, niter=3, warm=True)
        return (shape, *box(shape), pg, dict(op, warm=True), {}, "myula_step_pipe_kernel(warm)", 2)
    raise KeyError(name)


FAMILIES = ["tile", "tile_aniso", "point", "block", "rows", "split", "pipe", "pipe_aniso", "pipe2", "pipe_chained", "pipe_warm"]


@pytest.mark.parametrize("name", FAMILIES)
def test_myula_families_injected_noise_every_chain(la, name):
    """one or two steps of 65543 chains with tiled states and tiled injected noise against the checker's 7 results"""
    shape, pf, (y, h, off, mask), pg, op, kw, kernel, nit = family(la, name)
    rng = np.random.default_rng(21)
    x7 = M.patterns(shape, 20)
    noise7 = rng.standard_normal((nit, P) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C, tau=TAU, gamma=GAMMA, noise="injected", **kw)
    smp.set_state(M.tile_dev(x7, C))
    ref = x7
    for it in range(nit):
        smp.step(1, noise=M.tile_dev(noise7[it], C)[None])
        ref = M.myula_step_ref(ref, y, h, off, TAU, GAMMA, op, noise7[it], mask=mask)
    print(f"{name} {shape}: {smp.kernel_name}")
    assert smp.kernel_name == kernel, smp.kernel_name
    got = smp.get_state()
    M.check_per_image(got, ref, 5e-6 * nit if nit > 1 else STEP_TOL, f"MYULA {name}, injected noise, step {nit}")
    if name == "tile":               # energies() of the sampler, per chain, at the states it holds
        f, g = smp.energies()
        fo, go = O.energies(got[:P].cpu().numpy().astype(np.float64), y, h, off, SF, op)
        M.check_per_image(f, fo, STEP_TOL, "sampler energies f")
        M.check_per_image(g, go, STEP_TOL, "sampler energies g")
    smp.close()


def test_block_kernel_with_the_mc_tv_term_every_chain(la):
    """mask + Haar-l1 + the MC-TV term: the block kernel, then mc_tv_add with tiles * n_img workgroups"""
    shape = (8, 8)
    rng = np.random.default_rng(22)
    mask = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    b = (mask * (M.patterns(shape, 23, noise=0.0)[3] + rng.normal(0, SIGMA, shape))).ravel()
    kw = dict(dims=shape, b=b, sigma=SF, lamda=TAU_REG, gamma=15.0, isotropic=True)
    pf = la.L2_ncvx_tv(Op=la.Diagonal(mask, dims=shape), Op2=la.Gradient(shape), **kw)
    of = O.L2NcvxTV(Op=O.Diagonal(mask.ravel()), Op2=O.Gradient(shape), **kw)
    x7, xi7 = M.patterns(shape, 24), rng.standard_normal((P,) + shape)
    smp = la.MYULASampler(pf, la.WaveletL1(shape, sigma=TAU_REG), shape, n_chains=C, tau=TAU, gamma=GAMMA, noise="injected")
    smp.set_state(M.tile_dev(x7, C))
    smp.step(1, noise=M.tile_dev(xi7, C)[None])
    assert smp.kernel_name == "myula_step_block_kernel", smp.kernel_name
    grad = np.stack([of.grad(x.ravel()).reshape(shape) for x in x7])
    ref = (1 - TAU / GAMMA) * x7 - TAU * grad + (TAU / GAMMA) * O.haar_l1_prox(x7, GAMMA * TAU_REG) + np.sqrt(2 * TAU) * xi7
    M.check_per_image(smp.get_state(), ref, STEP_TOL, "MYULA block kernel + MC-TV term")
    smp.close()


def test_per_chain_prox_scale_every_chain(la):
    """array-valued epsg, one weight per chain (strides (1, 0)): launch_prior_prox_scaled before every step"""
    shape = (5, 7)
    rng = np.random.default_rng(25)
    y = M.patterns(shape, 26)[2]
    x7, xi7 = M.patterns(shape, 27), rng.standard_normal((P,) + shape)
    e7 = np.linspace(0.5, 30.0, P)
    smp = la.MYULASampler(la.L2(b=y, sigma=SF, dims=shape), la.L1(sigma=0.4), shape, n_chains=C, tau=TAU, gamma=GAMMA, epsg=M.tile(e7, C), noise="injected")
    smp.set_state(M.tile_dev(x7, C))
    smp.step(1, noise=M.tile_dev(xi7, C)[None])
    ref = np.stack([M.myula_step_ref(x7[k], y, None, None, TAU, GAMMA, {"kind": "l1", "sigma": 0.4, "t": e7[k] * GAMMA}, xi7[k]) for k in range(P)])
    assert smp.kernel_name == "myula_step_split_kernel", smp.kernel_name      # the prox is its own launch, consumed by the split kernel
    M.check_per_image(smp.get_state(), ref, STEP_TOL, "MYULA with per-chain epsg")
    smp.close()


PHILOX = {"tile": 1, "point": 1, "block": 1, "block2": 2, "rows": 1, "rows_pair": 2, "split": 1, "pipe": 1, "pipe_aniso": 1, "pipe2": 1, "pipe_chained": 1, "pipe_warm": 2}


@pytest.mark.parametrize("name", list(PHILOX))
def test_myula_families_philox_windows_and_sharding(la, name):
    """Philox noise keyed by the global chain id, 65543 chains from chain_offset 4096: the field of iteration 0 against the checker for every chain;
    the chains on both sides of the 65535 seam, the first and the last four against the checker driven by its own Philox field, and bit for bit
    against the same chains run as a small batch of their own.  block2 / rows_pair: two iterations in one launch."""
    import torch
    nit = PHILOX[name]
    fam = {"block2": "block", "rows_pair": "rows"}.get(name, name)
    shape, pf, (y, h, off, mask), pg, op, kw, kernel, _ = family(la, fam)
    if name in ("block2", "rows_pair"):
        kw = dict(policy={"iterations_per_launch": 2})
        kernel = "myula_step_block_kernel(2 iterations)" if name == "block2" else "myula_step_rows_pair_kernel"
    seed, base = 0x5DEECE66D1234567, 4096
    x7 = M.patterns(shape, 30)
    mk = lambda n, first: la.MYULASampler(pf, pg, shape, n_chains=n, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=base + first, **kw)
    big = mk(C, 0)
    big.set_state(M.tile_dev(x7, C))
    xi = big.noise_field(0)
    worst, at = 0.0, 0
    for a in range(0, C, 8192):           # every chain's field of iteration 0
        b = min(a + 8192, C)
        d = np.abs(xi[a:b].cpu().numpy() - O.philox_normals(seed, 0, base + np.arange(a, b), *shape)).max(axis=(1, 2))
        if d.max() > worst:
            worst, at = float(d.max()), a + int(d.argmax())
    assert worst < NOISE_TOL, f"noise_field: chain {at} (index {at % M.CHUNK}) is off by {worst:.3e}"
    del xi
    big.step(nit)
    print(f"{name} {shape}: {big.kernel_name}")
    assert big.kernel_name == kernel, big.kernel_name
    w = M.windows(C)
    got = big.get_state()[torch.from_numpy(w).to("cuda")]
    big.close()
    ref = x7[w % P]
    opw = dict(op)
    for it in range(nit):
        ref = M.myula_step_ref(ref, y, h, off, TAU, GAMMA, opw, O.philox_normals(seed, it, base + w, *shape).astype(np.float64), mask=mask)
    e, i = M.worst(M.per_image_rel(got, ref))
    print(f"{name}: worst window chain {w[i]} rel {e:.3e}")
    assert e < (5e-6 * nit if nit > 1 else STEP_TOL), f"MYULA {name}, Philox: chain {w[i]} (index {w[i] % M.CHUNK}) is off by rel {e:.3e}"
    for first, last in ((0, 4), (M.CHUNK - 4, M.CHUNK + 5), (C - 4, C)):      # the same chains on their own
        sel = np.arange(first, last)
        solo = mk(len(sel), first)
        solo.set_state(np.ascontiguousarray(x7[sel % P], dtype=np.float32))
        solo.step(nit)
        pos = torch.from_numpy(np.searchsorted(w, sel)).to("cuda")
        same = torch.equal(solo.get_state(), got[pos])
        solo.close()
        assert same, f"MYULA {name}: chains {first}..{last - 1} differ from the same chains run alone"


# =========================================================================================== moments
@pytest.mark.parametrize("shape", [(4, 6), (5, 7)])
@pytest.mark.parametrize("overlap", [0, -1])
def test_moments_over_65543_chains(la, shape, overlap):
    """burn_in = 1, thin = 2 over 4 steps in ONE call (so the reductions run beside the next launches where the policy allows): sum and sum of
    squares of the kept iterates against fp64 torch sums of the states of a twin sampler stepped one iteration at a time"""
    x7 = M.patterns(shape, 31)
    y = M.patterns(shape, 32)[4]
    pf, pg = la.L2(b=y, sigma=SF, dims=shape), la.L1(sigma=0.4)
    mk = lambda mom, pol: la.MYULASampler(pf, pg, shape, n_chains=C, tau=TAU, gamma=GAMMA, seed=41, chain_offset=17, moments=mom, burn_in=1, thin=2, policy=pol)
    a, b = mk(True, {"moments_overlap": overlap}), mk(False, None)
    for s in (a, b):
        s.set_state(M.tile_dev(x7, C))
    a.step(4)
    import torch
    t1 = torch.zeros(shape, dtype=torch.float64, device="cuda")
    t2 = torch.zeros_like(t1)
    kept = 0
    for k in range(4):
        b.step(1)
        if k >= 1 and (k - 1) % 2 == 0:
            xs = b.get_state().double()
            t1 += xs.sum(dim=0)
            t2 += (xs * xs).sum(dim=0)
            kept += 1
    assert kept == 2 and torch.equal(a.get_state(), b.get_state())
    s1, s2, n = a.moments()
    print(f"moments {shape} overlap={overlap}: {a.kernel_name}, count {n}, rel {M.global_rel(s1.cpu().numpy(), t1.cpu().numpy()):.2e} {M.global_rel(s2.cpu().numpy(), t2.cpu().numpy()):.2e}")
    assert a.kernel_name == "myula_step_split_kernel" and b.kernel_name == a.kernel_name, (a.kernel_name, b.kernel_name)
    assert n == kept * C
    assert M.global_rel(s1.cpu().numpy(), t1.cpu().numpy()) < 1e-9
    assert M.global_rel(s2.cpu().numpy(), t2.cpu().numpy()) < 1e-9
    a.close()
    b.close()


# =========================================================================================== ULPDA
ULPDA_AMP = 0.04       # grey levels of the ULPDA scenes: up to about 10 instead of 255 (see test_ulpda_every_chain_and_philox_windows)


def ulpda_problem(la, data, shape):
    """(device data term, checker data term factory)"""
    if data == "identity":
        b = ULPDA_AMP * M.patterns(shape, 33)[1]
        return la.L2(b=b, sigma=SF, dims=shape), lambda: O.L2(b=b.ravel(), sigma=SF)
    h, off = (np.ones((5, 5)) / 25, (2, 2)) if data == "cheb" else (M.H3_NONSEP, (1, 1))
    y = O.blur(ULPDA_AMP * M.patterns(shape, 34, noise=0.0)[3], h, off) + np.random.default_rng(35).normal(0, SIGMA, shape)
    return (la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y.ravel(), sigma=SF, niter=50, warm=True),
            lambda: O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=SF, niter=60, warm=True))


ULPDA_TAU, ULPDA_MU = 0.95 * SIGMA ** 2, 0.99 / (0.95 * SIGMA ** 2 * 8)
ULPDA_NAMES = {"identity": "ulpda (multi-kernel)", "cg": "ulpda (multi-kernel)", "cheb": "ulpda (multi-kernel)", "cheb_pair": "ulpda (multi-kernel, chebyshev pairs)"}


@pytest.mark.parametrize("gfirst", [False, True])
@pytest.mark.parametrize("iso", [True, False])
@pytest.mark.parametrize("data", ["identity", "cg", "cheb", "cheb_pair"])
def test_ulpda_every_chain_and_philox_windows(la, monkeypatch, data, iso, gfirst):
    """ULPDA at 8 x 8 with 65543 chains, two iterations: ulpda_dual4 / ulpda_rhs4 / ulpda_finish_philox over chunks of 65535 chains, the implicit
    data step by CG (non-separable 3 x 3), Chebyshev (5 x 5 box), Chebyshev two iterations per launch, or pointwise.  Injected tiled noise: state
    and dual of every chain; Philox: the window chains against the checker.  The implicit solves stop at a relative residual of 1e-7 (see
    test_l2_implicit_step_past_two_chunks).

    Grey levels up to about 10 (ULPDA_AMP), not 255: the dual is the projection of y + mu A xhat onto a ball of radius 0.3, so a rounding error of
    the state, eps32 x amplitude per pixel, reaches an unsaturated dual entry as mu x 6 x eps32 x amplitude / 0.3 (xhat = 2 x - x_old, a difference
    of two pixels) -- an estimate of 7e-5 at amplitude 255 for any fp32 kernel.  Measured on the MI355X with scenes of amplitude 255: state 2e-7, dual
    1.47e-5 (non-separable blur, L21, gfirst) against the 1e-5 asked for here; at amplitude 10 the same rounding stays below 3e-6, and more of
    the dual field lies inside the ball, so both branches of the projection are compared."""
    import torch
    shape, nit = (8, 8), 2
    n = shape[0] * shape[1]
    # iterations per launch of the Chebyshev solve: 2 = pairs wherever the kernel covers the problem, 1 = single launches (the default pairs up
    # where it pays, C H >= 2^17 -- which 65543 x 8 is, but the window chains on their own are not)
    monkeypatch.setenv("LMC_CHEB_PAIR", "2" if data == "cheb_pair" else "0")
    pf, mk_of = ulpda_problem(la, "cheb" if data == "cheb_pair" else data, shape)
    pg, og = (la.L21(sigma=TAU_REG), O.L21(sigma=TAU_REG)) if iso else (la.L1(sigma=TAU_REG), O.L1(sigma=TAU_REG))
    G, Go = la.Gradient(shape), O.Gradient(shape)
    x7 = ULPDA_AMP * M.patterns(shape, 36)
    rng = np.random.default_rng(37)
    noise7 = rng.standard_normal((nit, P, n))
    mk = lambda mode, **kw: la.ULPDASampler(pf, pg, G, shape, n_chains=C, tau=ULPDA_TAU, mu=ULPDA_MU, theta=1.0, gfirst=gfirst, noise=mode, implicit_tol=1e-7, **kw)

    def checker(x0, noise):
        xs, ys = O.ulpda(mk_of(), og, Go, x0.ravel(), ULPDA_TAU, ULPDA_MU, theta=1.0, niter=nit, gfirst=gfirst, returny=True, noise=noise)
        return xs[-1], ys[-1]

    smp = mk("injected")
    smp.set_state(M.tile_dev(x7, C))
    for it in range(nit):
        smp.step(1, noise=M.tile_dev(noise7[it].reshape((P,) + shape), C)[None])
    assert smp.kernel_name == ULPDA_NAMES[data], smp.kernel_name
    ref = [checker(x7[k], noise7[:, k]) for k in range(P)]
    tag = f"ULPDA {data} {'L21' if iso else 'L1'} gfirst={gfirst}"
    M.check_per_image(smp.get_state(), np.stack([r[0] for r in ref]), 5e-6 * nit, tag + ", injected noise, state")
    M.check_per_image(smp.get_dual(), np.stack([r[1] for r in ref]), 5e-6 * nit, tag + ", injected noise, dual")
    smp.close()
    torch.cuda.empty_cache()
    seed, base = 77, 4096
    smp = mk("philox", seed=seed, chain_offset=base)
    smp.set_state(M.tile_dev(x7, C))
    smp.step(nit)
    w = M.windows(C)
    idx = torch.from_numpy(w).to("cuda")
    gx, gy = smp.get_state()[idx], smp.get_dual()[idx]
    smp.close()
    ref = [checker(x7[c % P], np.stack([O.philox_normals(seed, it, [base + c], *shape)[0].ravel().astype(np.float64) for it in range(nit)])) for c in w]
    for got, k, what in ((gx, 0, "state"), (gy, 1, "dual")):
        e, i = M.worst(M.per_image_rel(got, np.stack([r[k] for r in ref])))
        print(f"{tag}, Philox, {what}: worst window chain {w[i]} rel {e:.3e}")
        assert e < 5e-6 * nit, f"{tag}, Philox: {what} of chain {w[i]} (index {w[i] % M.CHUNK}) is off by rel {e:.3e}"


# =========================================================================================== MYMALA
def test_mymala_one_step_every_chain(la):
    """8 x 8, tiled states and injected noise, the Metropolis uniforms from Philox by global chain id: log alpha of every chain; accept flag and
    state of the chains whose decision the fp32 energies cannot flip (tests/test_gpu_mymala.py's margin) -- over 95 % of them, with both outcomes"""
    shape, off_c = M.MALA_SHAPE, 40
    y, h, off, prior, x7, xi7 = M.mala_scene()
    la_o, logu, ok, safe, xp, x0, bound = M.mala_reference(off_c + np.arange(C))
    assert safe.mean() >= 0.95 and ok[safe].any() and (~ok[safe]).any(), (safe.mean(), ok.mean())
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=SF)
    smp = la.MYMALASampler(pf, la.TV(shape, sigma=TAU_REG, niter=10), shape, n_chains=C, tau=M.MALA_TAU, gamma=GAMMA, noise="injected", seed=M.MALA_SEED,
                           chain_offset=off_c)
    smp.set_state(M.tile_dev(x7, C))
    smp.step(1, noise=M.tile_dev(xi7, C)[None])
    acc_d, la_d = smp.acceptance()
    acc_d, la_d = acc_d.cpu().numpy(), la_d.cpu().numpy()
    got = smp.get_state().cpu().numpy()
    print(f"MYMALA: {smp.kernel_name}; safe {safe.mean():.4f}, accepted {ok.mean():.4f} (device {acc_d.mean():.4f})")
    assert smp.kernel_name == "myula_step_split_kernel", smp.kernel_name
    smp.close()
    err = np.abs(la_d - M.tile(la_o, C))
    i = int(err.argmax())
    assert err[i] < bound, f"log alpha of chain {i} (index {i % M.CHUNK}) is off by {err[i]:.3e} >= {bound:.3e}"
    bad = np.flatnonzero(safe & (acc_d.astype(bool) != ok))
    assert bad.size == 0, f"{bad.size} clear-cut chains decided the other way, first: chain {bad[0]} (index {bad[0] % M.CHUNK})"
    want = np.where(ok[:, None, None], M.tile(xp, C), M.tile(x0, C))
    errs = np.where(safe, M.per_image_rel(got, want), 0.0)
    e, i = M.worst(errs)
    assert e < STEP_TOL, f"state of chain {i} (index {i % M.CHUNK}, accepted={bool(ok[i])}) is off by rel {e:.3e}"


# =========================================================================================== chain ids at the top of the 32-bit range
def test_chain_ids_at_the_top_of_the_range(la):
    """chain_offset = 2^32 - 1 - C: the Philox counter word of the chain runs up to 2^32 - 2 without wrapping; one more is refused"""
    import torch
    shape, seed = (4, 8), 99
    base = 2 ** 32 - 1 - C
    x7 = M.patterns(shape, 40)
    h, off, y = M.blur_problem(shape, 5)
    pf, (_, _, _, mask) = blur_terms(la, shape, h, off, y)
    op = {"kind": "l1", "sigma": 0.4, "t": GAMMA}
    smp = la.MYULASampler(pf, la.L1(sigma=0.4), shape, n_chains=C, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=base)
    smp.set_state(M.tile_dev(x7, C))
    w = M.windows(C)
    idx = torch.from_numpy(w).to("cuda")
    ids = (base + w).astype(np.uint64)
    assert int(ids.max()) == 2 ** 32 - 2
    for it in (0, 3):
        d = np.abs(smp.noise_field(it)[idx].cpu().numpy() - O.philox_normals(seed, it, ids, *shape))
        assert d.max() < NOISE_TOL, (it, int(w[d.max(axis=(1, 2)).argmax()]), float(d.max()))
    smp.step(1)
    assert smp.kernel_name == "myula_step_rows_kernel", smp.kernel_name
    ref = M.myula_step_ref(x7[w % P], y, h, off, TAU, GAMMA, op, O.philox_normals(seed, 0, ids, *shape).astype(np.float64))
    e, i = M.worst(M.per_image_rel(smp.get_state()[idx], ref))
    assert e < STEP_TOL, f"chain {w[i]} (global id {ids[i]}) is off by rel {e:.3e}"
    # the last chain alone, with its global id
    one = la.MYULASampler(pf, la.L1(sigma=0.4), shape, n_chains=1, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=2 ** 32 - 2)
    one.set_state(np.ascontiguousarray(x7[(C - 1) % P], dtype=np.float32))
    one.step(1)
    assert torch.equal(one.get_state()[0], smp.get_state()[C - 1])
    one.close()
    smp.close()
    with pytest.raises(la.LMCError):
        la.MYULASampler(pf, la.L1(sigma=0.4), shape, n_chains=C, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=2 ** 32 - C)


# =========================================================================================== the anisotropic ME-TV term (the defect fixed with these tests)
@pytest.mark.parametrize("rtol", [0.0, 1e-4])
def test_me_tv_aniso_term_past_65535_images(la, rtol):
    """L2_ncvx_tv(isotropic=False, Op2=None): f(x) = sigma/2 ||x - b||^2 - lamda env_gamma(TV_1D)(x) on 4 x 6 images.  Its inner prox is a 1-D TV over
    the flattened image, one launch per dual iteration with the images on gridDim.y; above 65535 images those launches were refused with
    hipErrorInvalidConfiguration (LMC_E_HIP in the middle of a step).  Gradient of 131077 images and one MYULA step of 65543 chains against the
    checker's 1-D FGP, with and without the early exit."""
    shape, lam, gam, niter = (4, 6), 0.3, 5.0, 20          # rtol = 1e-4: six of the seven patterns leave early, visibly (1e-4 of the prox)
    n = shape[0] * shape[1]
    x7 = M.rtol_patterns(shape) + 40.0
    rng = np.random.default_rng(50)
    b = x7[2] + rng.normal(0, SIGMA, shape)
    pf = la.L2_ncvx_tv(dims=shape, Op=la.Identity(n), Op2=None, b=b.ravel(), sigma=SF, lamda=lam, gamma=gam, isotropic=False, niter=niter, rtol=rtol)
    prox = np.stack([O.tv1d_prox_fgp(x.ravel(), gam, niter, step=0.25, rtol=rtol).reshape(shape) for x in x7])
    if rtol > 0:                      # the exit is taken, and in different passes
        fixed = np.stack([O.tv1d_prox_fgp(x.ravel(), gam, niter, step=0.25).reshape(shape) for x in x7])
        assert sum(not np.array_equal(p, q) for p, q in zip(prox, fixed)) >= 2
    grad = SF * (x7 - b) - lam * (x7 - prox) / gam
    M.check_per_image(pf.grad(M.tile_dev(x7, N).reshape(N, -1)), grad, STEP_TOL, f"L2_ncvx_tv anisotropic ME-TV gradient, rtol={rtol}")
    xi7 = rng.standard_normal((P,) + shape)
    smp = la.MYULASampler(pf, None, shape, n_chains=C, tau=TAU, gamma=GAMMA, noise="injected")
    smp.set_state(M.tile_dev(x7, C))
    smp.step(1, noise=M.tile_dev(xi7, C)[None])
    assert smp.kernel_name == "myula_step_split_kernel", smp.kernel_name     # the fused step; the inner 1-D prox is the tv1d launches before it
    ref = x7 - TAU * grad + np.sqrt(2 * TAU) * xi7          # no prior: prox = identity, (1 - tau/gamma) x + (tau/gamma) x
    M.check_per_image(smp.get_state(), ref, STEP_TOL, f"MYULA step with the anisotropic ME-TV term, rtol={rtol}")
    f, _ = smp.energies()
    x1 = smp.get_state()[:P].cpu().numpy().astype(np.float64)
    p1 = np.stack([O.tv1d_prox_fgp(x.ravel(), gam, niter, step=0.25, rtol=rtol).reshape(shape) for x in x1])
    env = O.tv1d_value(p1.reshape(P, -1)) + np.sum((x1 - p1) ** 2, axis=(1, 2)) / (2 * gam)
    M.check_per_image(f, 0.5 * SF * np.sum((x1 - b) ** 2, axis=(1, 2)) - lam * env, STEP_TOL, f"energies with the anisotropic ME-TV term, rtol={rtol}")
    smp.close()
