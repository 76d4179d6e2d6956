"""Images thinner than a kernel's own footprint: 1 to 4 rows for the row pipelines (whose prologues clamp their row loads with
min(max(r, 0), H - 1) and whose lag is longer than the image), 1 to 3 columns for everything that takes them.  The coverage tests of the
kernels accept H >= 1, but only the isotropic pipe kernel was run on images shorter than its prefetch depth (tests/test_gpu_pipe.py,
tests/test_gpu_pipe_teams.py); the smallest heights elsewhere were 20 (anisotropic pipe, rt early exit), 18 (column strips), 37 (rows-pair) and 8
(ULPDA's implicit step).

Three chains, one or two steps with injected noise (Philox where a kernel takes nothing else) against the checker at the project's tolerances
(1e-5 for one operator / one step, 5e-6 x steps along a trajectory), with the kernel that ran asserted."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
from tests import _many as M

pytestmark = pytest.mark.gpu

STEP_TOL, SIGMA, TAU_REG, GAMMA, TAU = M.STEP_TOL, M.SIGMA, M.TAU_REG, M.GAMMA, M.TAU
SF = 1 / SIGMA ** 2
HS = [1, 2, 3, 4]
NC = 3


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")


def blur_terms(la, shape, k=5):
    h, off, y = M.blur_problem(shape, k, seed=shape[0] + shape[1])
    return la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=SF), (y, h, off)


def run_injected(la, shape, pf, dat, pg, op, kernel, nit=2, **kw):
    """`nit` single steps of NC chains with injected noise, each against the checker; returns the sampler (open) and the final reference"""
    y, h, off = dat
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = M.patterns(shape, 3)[:NC]
    noise = rng.standard_normal((nit, NC) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=NC, tau=TAU, gamma=GAMMA, noise="injected", **kw)
    smp.set_state(x)
    for it in range(nit):
        smp.step(1, noise=noise[it:it + 1])
        x = M.myula_step_ref(x, y, h, off, TAU, GAMMA, op, noise[it])
        e, c = M.worst(M.per_image_rel(smp.get_state(), x))
        print(f"{shape} {smp.kernel_name} step {it + 1}: worst chain {c} rel {e:.3e}")
        assert e < (STEP_TOL if it == 0 else 5e-6 * (it + 1)), (shape, smp.kernel_name, it, c, e)
    assert kernel in smp.kernel_name, (shape, smp.kernel_name)
    return smp, x


# ------------------------------------------------------------------ the full-width pipeline
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("W", [136, 203, 264, 520])
@pytest.mark.parametrize("niter", [10, 20])
def test_anisotropic_pipe_on_thin_images(la, niter, W, H):
    """one launch (10 dual iterations) and a chain of two (20); 203: unaligned rows; 520: two column strips"""
    shape = (H, W)
    pf, dat = blur_terms(la, shape)
    op = {"kind": "tv_aniso", "sigma": TAU_REG, "niter": niter, "t": GAMMA}
    run_injected(la, shape, pf, dat, la.TV(shape, sigma=TAU_REG, niter=niter, isotropic=False), op, "myula_step_pipe_aniso_kernel")[0].close()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("W", [520, 877])
def test_isotropic_pipe_on_thin_column_strips(la, W, H):
    shape = (H, W)
    pf, dat = blur_terms(la, shape)
    op = {"kind": "tv", "sigma": TAU_REG, "niter": 10, "t": GAMMA}
    smp, _ = run_injected(la, shape, pf, dat, la.TV(shape, sigma=TAU_REG, niter=10), op, "myula_step_pipe_kernel")
    assert smp.kernel_name == "myula_step_pipe_kernel"
    smp.close()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("W", [136, 520])
def test_device_side_early_exit_on_thin_images(la, W, H):
    """TV(rtol = 1e-4) decided on the device inside the fused launch: states against the checker's rtol branch, and the pass every chain left in.
    One-row images of this scene run out of passes at sigma = 0.3 (in the checker): they take sigma = 0.05, where the chains leave in passes 4 to 10."""
    shape = (H, W)
    pf, (y, h, off) = blur_terms(la, shape)
    sig = 0.05 if H == 1 else TAU_REG
    rng = np.random.default_rng(H * 1000 + W)
    x = M.rtol_patterns(shape)[[0, 1, 5]]                       # the zero image (runs out of passes), a quiet and a noisy one
    noise = rng.standard_normal((2, NC) + shape)
    smp = la.MYULASampler(pf, la.TV(shape, sigma=sig, niter=10, rtol=M.RTOL), shape, n_chains=NC, tau=TAU, gamma=GAMMA, noise="injected")
    smp.set_state(x)
    seen = set()
    for it in range(2):
        res = [M.tv_prox_exit(xc, sig * GAMMA, 10, M.RTOL) for xc in x]
        passes = np.array([r[1] for r in res])
        seen |= set(passes.tolist())
        smp.step(1, noise=noise[it:it + 1])
        assert "per-chain exit" in smp.kernel_name, smp.kernel_name
        ps, reruns = smp.tv_exit_stats("prior")
        np.testing.assert_array_equal(ps.cpu().numpy(), passes)
        assert reruns[3] == 0
        x = M.myula_step_ref(x, y, h, off, TAU, GAMMA, {"kind": "none"}, noise[it]) + (TAU / GAMMA) * (np.stack([r[0] for r in res]) - x)
        e, c = M.worst(M.per_image_rel(smp.get_state(), x))
        print(f"{shape} step {it + 1}: passes {passes.tolist()}, worst chain {c} rel {e:.3e}")
        assert e < (STEP_TOL if it == 0 else 5e-6 * (it + 1)), (shape, it, c, e)
    assert len(seen) >= 3, seen
    smp.close()


# ------------------------------------------------------------------ row streaming
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("W", [8, 260, 520])
def test_rows_kernel_on_thin_images(la, W, H):
    """separable blur + l1: one wave per band of rows; 520: two column strips"""
    shape = (H, W)
    pf, dat = blur_terms(la, shape)
    op = {"kind": "l1", "sigma": 0.4, "t": GAMMA}
    run_injected(la, shape, pf, dat, la.L1(sigma=0.4), op, "myula_step_rows_kernel", policy={"iterations_per_launch": 1})[0].close()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("W", [8, 260, 520])
def test_rows_pair_kernel_on_thin_images(la, W, H):
    """two iterations per launch (Philox only): up to 512 columns the pair kernel, which re-reads rows of neighbouring bands; 520 is beyond it and
    must run the single-iteration kernel, not something in between"""
    shape = (H, W)
    pf, (y, h, off) = blur_terms(la, shape)
    op = {"kind": "l1", "sigma": 0.4, "t": GAMMA}
    seed, base = 5, 11
    x = M.patterns(shape, 3)[:NC]
    smp = la.MYULASampler(pf, la.L1(sigma=0.4), shape, n_chains=NC, tau=TAU, gamma=GAMMA, seed=seed, chain_offset=base, policy={"iterations_per_launch": 2})
    smp.set_state(x)
    smp.step(2)
    assert smp.kernel_name == ("myula_step_rows_pair_kernel" if W <= 512 else "myula_step_rows_kernel"), smp.kernel_name
    for it in range(2):
        x = M.myula_step_ref(x, y, h, off, TAU, GAMMA, op, O.philox_normals(seed, it, base + np.arange(NC), *shape).astype(np.float64))
    e, c = M.worst(M.per_image_rel(smp.get_state(), x))
    print(f"{shape} {smp.kernel_name}: worst chain {c} rel {e:.3e}")
    assert e < 5e-6 * 2, (shape, c, e)
    smp.close()


# ------------------------------------------------------------------ split and point kernels
@pytest.mark.parametrize("H", HS)
def test_split_kernel_on_thin_images(la, H):
    shape = (H, 96)
    pf, dat = blur_terms(la, shape)
    op = {"kind": "tv", "sigma": TAU_REG, "niter": 10, "t": GAMMA}
    run_injected(la, shape, pf, dat, la.TV(shape, sigma=TAU_REG, niter=10), op, "myula_step_split_kernel", variant="split")[0].close()


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("data", ["identity", "blur"])
def test_point_kernel_on_thin_images(la, data, H):
    shape = (H, 203)
    if data == "blur":
        pf, dat = blur_terms(la, shape)
    else:
        y = M.patterns(shape, 6)[4]
        pf, dat = la.L2(b=y, sigma=SF, dims=shape), (y, None, None)
    op = {"kind": "l1", "sigma": 0.4, "t": GAMMA}
    run_injected(la, shape, pf, dat, la.L1(sigma=0.4), op, "myula_step_point_kernel", variant="point")[0].close()


# ------------------------------------------------------------------ ULPDA: the Chebyshev solve of the implicit step, single launches and pairs
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("pair", [False, True])
def test_ulpda_chebyshev_on_thin_images(la, monkeypatch, pair, H):
    """5 x 5 box on H x 136: the implicit data step by the row-streaming Chebyshev iteration, one or two iterations per launch, stopped at a
    relative residual of 1e-7 (the default 1e-6 leaves more than the 1e-5 asked for here; tests/test_gpu_ulpda.py allows 2e-5 to 1e-4 with it)"""
    shape, nit = (H, 136), 2
    n = H * 136
    monkeypatch.setenv("LMC_CHEB_PAIR", "2" if pair else "0")
    amp = 0.04                                                   # grey levels up to about 10: see test_ulpda_every_chain_and_philox_windows
    h, off = np.ones((5, 5)) / 25, (2, 2)
    y = O.blur(amp * M.patterns(shape, H, noise=0.0)[3], h, off) + np.random.default_rng(H + 100).normal(0, SIGMA, shape)
    tau, mu = 0.95 * SIGMA ** 2, 0.99 / (0.95 * SIGMA ** 2 * 8)
    rng = np.random.default_rng(H)
    x0 = amp * M.patterns(shape, 7)[:NC]
    noise = rng.standard_normal((nit, NC, n))
    for gfirst in (False, True):
        l2 = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y.ravel(), sigma=SF, niter=50, warm=True)
        smp = la.ULPDASampler(l2, la.L21(sigma=TAU_REG), la.Gradient(shape), shape, n_chains=NC, tau=tau, mu=mu, theta=1.0, gfirst=gfirst, noise="injected",
                              implicit_tol=1e-7)
        smp.set_state(x0)
        smp.step(nit, noise=noise.reshape((nit, NC) + shape))
        assert smp.kernel_name == ("ulpda (multi-kernel, chebyshev pairs)" if pair else "ulpda (multi-kernel)"), smp.kernel_name
        gx, gy = smp.get_state().cpu().numpy(), smp.get_dual().cpu().numpy()
        smp.close()
        for c in range(NC):
            l2o = O.L2(Op=O.Convolve2D(shape, h, off), b=y.ravel(), sigma=SF, niter=60, warm=True)
            xs, ys = O.ulpda(l2o, O.L21(sigma=TAU_REG), O.Gradient(shape), x0[c].ravel(), tau, mu, theta=1.0, niter=nit, gfirst=gfirst, returny=True,
                             noise=noise[:, c])
            ex, ey = M.global_rel(gx[c].ravel(), xs[-1]), M.global_rel(gy[c].ravel(), ys[-1])
            print(f"{shape} pair={pair} gfirst={gfirst} chain {c}: state {ex:.3e} dual {ey:.3e}")
            assert ex < 5e-6 * nit and ey < 5e-6 * nit, (shape, pair, gfirst, c, ex, ey)


# ------------------------------------------------------------------ one to three columns
NARROW = [(H, W) for H in (1, 5) for W in (1, 2, 3)]


@pytest.mark.parametrize("shape", NARROW + [(3, 2)])
def test_stateless_operators_on_narrow_images(la, shape):
    """blur (3 x 3 off centre, and 7 x 7 -- larger than the image), gradient, both TV proxes, Haar-free energies"""
    x = M.patterns(shape, 8)[:NC]
    flat = x.reshape(NC, -1)
    for h, off in ((M.H3_NONSEP, (0, 2)), (np.outer(np.arange(1.0, 8.0), np.arange(2.0, 9.0)) / 1000.0, (3, 3))):
        Op = la.Convolve2D(shape, h, offset=off)
        assert M.per_image_rel(Op.matvec(flat), O.blur(x, h, off)).max() < STEP_TOL, (shape, h.shape)
        assert M.per_image_rel(Op.rmatvec(flat), O.blur_adjoint(x, h, off)).max() < STEP_TOL, (shape, h.shape)
    G, Go = la.Gradient(shape), O.Gradient(shape)
    v = np.random.default_rng(9).normal(0, 0.4, (NC, 2 * flat.shape[1]))
    assert M.per_image_rel(G.matvec(flat), np.stack([Go.matvec(f) for f in flat])).max() < STEP_TOL
    assert M.per_image_rel(G.rmatvec(v), np.stack([Go.rmatvec(f) for f in v])).max() < STEP_TOL
    for iso in (True, False):
        out = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=iso).prox(x, GAMMA)
        ref = O.tv_prox_fgp(x, TAU_REG * GAMMA, 10) if iso else M.tv_prox_aniso(x, TAU_REG * GAMMA, 10)
        assert M.per_image_rel(out, ref).max() < STEP_TOL, (shape, iso)
    h, off = np.ones((7, 7)) / 49, (3, 3)
    y = O.blur(x[1], h, off)
    from lmc_atomi_amd.proximal import _Problem
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y + 1.0, sigma=SF)
    f, g = _Problem(shape, pf.descriptor(), la.TV(shape, sigma=TAU_REG).prior_descriptor()).energies(x)
    fo, go = O.energies(x, y + 1.0, h, off, SF, {"kind": "tv", "sigma": TAU_REG})
    assert M.per_image_rel(f, fo).max() < STEP_TOL and M.per_image_rel(g, go).max() < STEP_TOL, (shape, f, fo, g, go)     # (1 x 1: TV = 0 on both sides, exactly)
    # dual projections, soft threshold, and the implicit L2 step (7 x 7 box: Chebyshev from 4 columns on, CG below; solves stopped at 1e-7 as in
    # tests/test_gpu_many_images.py::test_l2_implicit_step_past_two_chunks)
    assert M.per_image_rel(la.L21(sigma=0.3).proxdual(v, 1.0), np.stack([O.L21(sigma=0.3).proxdual(f_, 1.0) for f_ in v])).max() < STEP_TOL
    assert M.per_image_rel(la.L1(sigma=0.3).proxdual(v, 1.0), np.clip(v, -0.3, 0.3)).max() < STEP_TOL
    assert M.per_image_rel(la.L1(sigma=0.3).prox(flat, 20.0), O.L1(sigma=0.3).prox(flat, 20.0)).max() < STEP_TOL
    prev = la.set_cg_tolerance(1e-7)
    try:
        out = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=(y + 1.0).ravel(), sigma=SF, niter=50, warm=False).prox(flat, 0.53)
    finally:
        la.set_cg_tolerance(prev)
    l2o = O.L2(Op=O.Convolve2D(shape, h, off), b=(y + 1.0).ravel(), sigma=SF, niter=60, warm=False)
    assert M.per_image_rel(out, np.stack([l2o.prox(f_, 0.53) for f_ in flat])).max() < STEP_TOL, shape


@pytest.mark.parametrize("shape", NARROW + [(3, 2)])
@pytest.mark.parametrize("prior", ["tv", "tv_aniso", "l1"])
def test_samplers_on_narrow_images(la, shape, prior):
    """what auto picks -- the split kernel, the LDS-tiled one for the anisotropic prior; 7 x 7 blur, larger than the image"""
    h, off = np.ones((7, 7)) / 49, (3, 3)
    y = O.blur(M.patterns(shape, 10, noise=0.0)[2], h, off) + np.random.default_rng(11).normal(0, SIGMA, shape)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=off), b=y, sigma=SF)
    if prior == "l1":
        pg, op = la.L1(sigma=0.4), {"kind": "l1", "sigma": 0.4, "t": GAMMA}
    else:
        pg, op = la.TV(shape, sigma=TAU_REG, niter=10, isotropic=prior == "tv"), {"kind": prior, "sigma": TAU_REG, "niter": 10, "t": GAMMA}
    smp, _ = run_injected(la, shape, pf, (y, h, off), pg, op, "myula_step_")
    assert smp.kernel_name == ("myula_step_tile_kernel" if prior == "tv_aniso" else "myula_step_split_kernel"), smp.kernel_name      # (no anisotropic split kernel)
    smp.close()
