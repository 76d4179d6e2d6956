"""GPU parity of the Huber data term (LMC_DATA_HUBER_* in include/lmc_atomi.h, `la.HuberLoss`) against the float64 reference of tests/_huber_ref.py,
case for case as tests/test_gpu_wl2.py: the gradient through `lmc_fused_eval`, the fused MYULA step in the tiled kernel (`myula_step_tile_hub_kernel` /
`myula_step_tile_hub_box_kernel`) and in the full-width pipeline (`myula_step_pipe_hub_kernel` / `myula_step_pipe_hub_box_kernel`), what falls back to
the tiled kernel, delta = +inf against the plain term, trajectories, the Philox path, chain sharding, SK-ROCK, SAPG, the energies, MYMALA's Metropolis
ratio, the large PSF, and the refusals of the C ABI and of the Python surface.

Tolerances are the project's: one operator or one step rel-L2 <= 1e-5, 1e-5 x (step index) along a trajectory, energies rtol 5e-5; MYMALA: log alpha
within 2e-6 max|U(x0)| + 2e-3, states rel-L2 2e-5 on the clear-cut chains (tests/test_gpu_wl2.py).  The gradient and the one-step cases are also held
per pixel to tests/_pixel.py's bound max(3 e32, 2 ulp32(max |ref64|)), e32 from `HuberRef`'s own float32 replay and never from a kernel; no pixel is
excluded (psi and h are continuous: a residual within rounding of +-delta costs only rounding).  Every comparison is against `HuberRef`, never against
another device path, except the one test that says so.  Every case first asserts, on the reference alone (`R.assert_discriminates`), that a fifth to
four fifths of the residuals are clipped, that delta = 0 and delta = +inf each hold >= 5 % of the pixels, and that the wrong kernels -- delta ignored,
the clamp after the adjoint, the clamp of Op x, the planes swapped, a multiplication by delta -- would miss the tolerance thirty- to a hundredfold."""
import ctypes as C
import functools

import numpy as np
import pytest

import _huber_ref as R
import _pixel as PX
import _psf_ref as PS
from oracle import lmc_oracle as O
from tests import _mala_ref as M

pytestmark = pytest.mark.gpu

STEP_TOL = R.STEP_TOL
ENERGY_RTOL = R.ENERGY_RTOL
STATE_TOL = 2e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
INF = R.INF
GAMMA, TV_WEIGHT, SIGMA_F = R.GAMMA, R.TV_WEIGHT, R.SIGMA_F
NONSEP = (np.array([[0.05, 0.2, 0.0], [0.1, 0.3, 0.15], [0.0, 0.05, 0.15]]), (0, 2))       # off-centre origin: not a centred separable blur
TAPS5 = np.array([0.1, 0.2, 0.4, 0.2, 0.1])                                                  # separable, centred, NOT uniform: the general blur wave


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


@functools.lru_cache(maxsize=None)
def case(shape, data="blur5", n_chains=2, edge=False):
    """(reference operator, y, delta, x0) of one configuration, computed once; read-only; float32 numbers.  `edge`: delta = 0 on the whole last column
    and last row."""
    if data == "taps5":
        op = R.Op("blur", np.outer(TAPS5, TAPS5), (2, 2))
    elif data.startswith("blur"):
        op = R.Op("blur", *R.box_kernel(int(data[4:])))
    elif data == "nonsep":
        op = R.Op("blur", *NONSEP)
    else:
        op = R.Op("identity")
    _, op, y, d, x0 = R.recipe(shape, n_chains=n_chains, op=op)
    if edge:
        d[:, -1] = 0.0
        d[-1, :] = 0.0
    for a in (y, d, x0):
        a.setflags(write=False)
    return op, y, d, x0


def device_op(la, shape, op):
    return la.Convolve2D(shape, op.args[0], offset=op.args[1]) if op.kind == "blur" else la.Identity(shape[0] * shape[1])


def device_term(la, shape, op, y, d, sigma=SIGMA_F):
    return la.HuberLoss(device_op(la, shape, op), y, d, sigma=sigma, dims=shape)


def priors(la, shape, prior, bounds, niter=10, iso=True, dtype=np.float64):
    if prior == "tv":
        return la.TV(shape, sigma=TV_WEIGHT, niter=niter, isotropic=iso, bounds=bounds), R.TVRef(shape, TV_WEIGHT, niter, bounds, aniso=not iso, dtype=dtype)
    if prior == "l1":
        return la.L1(sigma=0.2, bounds=bounds), R.SeparableRef(lambda v, t: O.L1(0.2).prox(v, t), bounds, dtype=dtype)
    if prior == "l2":
        return la.L2(sigma=0.05, dims=shape, bounds=bounds), R.SeparableRef(lambda v, t: v / v.dtype.type(1.0 + t * 0.05), bounds, dtype=dtype)
    if prior == "laplace":
        return la.Laplace(0.2, bounds=bounds), R.SeparableRef(lambda v, t: O.prox_laplace(v, t * 0.2), bounds, dtype=dtype)
    raise ValueError(prior)


def per_pixel(label, got, ref64, ref32):
    """Worst |got - ref64| as a fraction of the bound max(3 e32, 2 ulp32(max |ref64|)); printed, then asserted <= 1 over every chain and pixel."""
    ref32 = np.asarray(ref32)
    assert ref32.dtype == np.float32, ref32.dtype
    e32, bound = PX.bound_of(ref64, ref32)
    worst, where = PS.worst(got, ref64)
    print(f"per pixel {label}: worst {worst:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, fraction {worst / bound:.3f}")
    assert worst <= bound, (label, worst, bound, where)
    return worst / bound


# ------------------------------------------------------------------ 1. gradient
GRAD_CASES = [(data, shape) for shape in ((20, 33), (37, 150)) for data in ("blur5", "blur7", "nonsep", "identity")]


@pytest.mark.parametrize("data,shape", GRAD_CASES)
def test_gradient_matches_reference(la, data, shape):
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, sigma=1.3 * SIGMA_F)
    stats = R.assert_discriminates(ref, x0, STEP_TOL)
    pf = device_term(la, shape, op, y, d, sigma=1.3 * SIGMA_F)
    got = pf.grad(x0)
    assert got.shape == x0.shape
    want = ref.grad(x0)
    e = R.rel(got, want)
    print(f"grad {data} {shape}: rel {e:.3e}; clipped {stats[0]:.2f}, delta=0 {stats[1]:.2f}, delta=inf {stats[2]:.2f}, wrong gradients {stats[3]}")
    assert e < STEP_TOL, e
    per_pixel(f"grad {data} {shape}", got, want, R.HuberRef(op, y, d, sigma=1.3 * SIGMA_F, dtype=np.float32).grad(x0.astype(np.float32)))
    assert R.rel(pf.grad(x0[0].ravel()), ref.grad(x0[0]).ravel()) < STEP_TOL       # a flat image in, a flat gradient out


# ------------------------------------------------------------------ 2. one MYULA step, injected noise
def one_step(la, shape, data, bounds, variant, niter=10, iso=True, prior="tv", edge=False):
    """-> (rel-L2 of one injected-noise MYULA step against the reference, kernel name); asserts that the comparison discriminates and the per-pixel bound."""
    op, y, d, x0 = case(shape, data, edge=edge)
    ref = R.HuberRef(op, y, d, SIGMA_F)
    R.assert_discriminates(ref, x0, STEP_TOL)
    pf = device_term(la, shape, op, y, d)
    tau = R.step_size(ref)
    assert pf.grad_lipschitz() == pytest.approx(ref.grad_lipschitz(), rel=1e-6)
    pg, og = priors(la, shape, prior, bounds, niter, iso)
    xi = R.f32(np.random.default_rng(shape[1]).standard_normal(x0.shape))
    want = R.myula_step(ref, og, x0, tau, GAMMA, xi)
    smp = la.MYULASampler(pf, pg, shape, n_chains=x0.shape[0], tau=tau, gamma=GAMMA, noise="injected", variant=variant)
    smp.set_state(x0)
    smp.step(1, noise=xi[None])
    got = smp.get_state().cpu().numpy()
    name = smp.kernel_name
    smp.close()
    assert np.isfinite(got).all(), "NaN / inf in the state (masking of lanes past the row end?)"
    e = R.rel(got, want)
    if e < STEP_TOL:      # (a step that misses the rel-L2 tolerance is reported by the caller's assertion, with the kernel's name)
        _, og32 = priors(la, shape, prior, bounds, niter, iso, dtype=np.float32)
        w32 = R.myula_step(R.HuberRef(op, y, d, SIGMA_F, dtype=np.float32), og32, x0, tau, GAMMA, xi, dtype=np.float32)
        per_pixel(f"step {name} {data} {shape} bounds={bounds} {prior} K={niter} iso={iso}", got, want, w32)
    return e, name


@pytest.mark.parametrize("bounds", R.BOXES, ids=["free", "positive", "box"])
@pytest.mark.parametrize("data,shape", [("blur5", (20, 33)), ("blur5", (40, 128)), ("identity", (20, 33)), ("nonsep", (20, 33))])
def test_myula_step_tile(la, data, shape, bounds):
    e, name = one_step(la, shape, data, bounds, "auto")
    print(f"tile {data} {shape} bounds={bounds}: rel {e:.3e} ({name})")
    assert name == ("myula_step_tile_hub_box_kernel" if bounds else "myula_step_tile_hub_kernel"), name
    assert e < STEP_TOL, e


@pytest.mark.parametrize("shape,kw", [((24, 264), dict(iso=False)), ((24, 136), dict(niter=20)), ((24, 264), dict(niter=9)),
                                      ((24, 136), dict(prior="l1")), ((24, 264), dict(prior="l2")), ((24, 136), dict(prior="laplace"))],
                         ids=["aniso", "K20", "K9", "l1", "l2", "laplace"])
def test_fallbacks_run_the_tile_kernel(la, shape, kw):
    for bounds in (None, (0.0, 255.0)):
        e, name = one_step(la, shape, "blur5", bounds, "auto", **kw)
        print(f"fallback {kw} {shape} bounds={bounds}: rel {e:.3e} ({name})")
        assert name.startswith("myula_step_tile_hub"), name
        assert e < STEP_TOL, e


# shape -> what it reaches: PXL 4 aligned / lanes past the row end, PXL 8 aligned / past the row end, two strips
PIPE_CASES = [("blur5", (24, 136)), ("blur5", (24, 150)), ("blur5", (24, 264)), ("blur5", (24, 268)), ("blur5", (16, 520)), ("blur7", (24, 264)),
              ("identity", (24, 136))]


@pytest.mark.parametrize("bounds", R.BOXES, ids=["free", "positive", "box"])
@pytest.mark.parametrize("data,shape", PIPE_CASES)
def test_myula_step_pipe(la, data, shape, bounds):
    e, name = one_step(la, shape, data, bounds, "pipe")
    print(f"pipe {data} {shape} bounds={bounds}: rel {e:.3e} ({name})")
    assert name == ("myula_step_pipe_hub_box_kernel" if bounds else "myula_step_pipe_hub_kernel"), name
    assert e < STEP_TOL, e


def test_myula_step_pipe_with_an_unobserved_last_column_and_row(la):
    """delta = 0 on the whole last image column and last row at 24 x 150, where the last lanes reach past the row end."""
    e, name = one_step(la, (24, 150), "blur5", (0.0, 255.0), "pipe", edge=True)
    print(f"pipe edge thresholds: rel {e:.3e} ({name})")
    assert name == "myula_step_pipe_hub_box_kernel" and e < STEP_TOL, (name, e)


AUTO_KERNEL_24x264 = "myula_step_pipe_hub_box_kernel"      # DESIGN "Huber data term": the measured step times decide what auto picks


def test_tile_pipe_and_auto_agree_with_the_reference(la):
    e1, n1 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "tile")
    e7, n7 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "pipe")
    e0, n0 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "auto")
    print(f"24 x 264: tile {e1:.3e} ({n1}), pipe {e7:.3e} ({n7}), auto {e0:.3e} ({n0})")
    assert n1 == "myula_step_tile_hub_box_kernel" and n7 == "myula_step_pipe_hub_box_kernel"
    assert max(e1, e7, e0) < STEP_TOL
    assert n0 == AUTO_KERNEL_24x264, n0


def test_forced_pipe_on_an_uncovered_problem_raises(la):
    shape = (20, 33)
    op, y, d, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, d)
    kw = dict(n_chains=2, tau=1e-3, gamma=GAMMA, variant="pipe")
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, **kw)            # 33 columns
    shape = (24, 264)
    op, y, d, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, d)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10, isotropic=False), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=9), shape, **kw)


def test_lagged_output_of_eleven_is_ten_and_runs_the_pipe(la):
    shape = (24, 264)
    op, y, d, x0 = case(shape, "blur5")
    ref, pf = R.HuberRef(op, y, d, SIGMA_F), device_term(la, shape, op, y, d)
    tau = R.step_size(ref)
    xi = R.f32(np.random.default_rng(1).standard_normal(x0.shape))
    smp = la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=11, lagged_output=True), shape, n_chains=2, tau=tau, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    smp.step(1, noise=xi[None])
    e = R.rel(smp.get_state().cpu().numpy(), R.myula_step(ref, R.TVRef(shape, TV_WEIGHT, 10), x0, tau, GAMMA, xi))
    assert smp.kernel_name == "myula_step_pipe_hub_kernel" and e < STEP_TOL, (smp.kernel_name, e)
    smp.close()


# ------------------------------------------------------------------ 3. delta = +inf is the plain term (device against device: the one place)
@pytest.mark.parametrize("shape,data,variant,plain_kernel", [((20, 33), "blur5", "tile", "myula_step_tile_kernel"),
                                                              ((24, 264), "taps5", "pipe", "myula_step_pipe_kernel")])
def test_infinite_thresholds_are_the_plain_term(la, shape, data, variant, plain_kernel):
    """The pipe case has 5 taps that are not uniform, so the plain term runs the general form of the blur wave and not the uniform-box kernel."""
    op, y, _, x0 = case(shape, data)
    ref = R.HuberRef(op, y, INF, SIGMA_F)
    assert np.array_equal(ref.grad(x0), ref.grad_plain(x0))
    tau = R.step_size(ref)
    xi = R.f32(np.random.default_rng(2).standard_normal(x0.shape))
    want = R.myula_step(ref, R.TVRef(shape, TV_WEIGHT, 10), x0, tau, GAMMA, xi)
    got = {}
    for label, pf in [("huber", device_term(la, shape, op, y, INF)), ("plain", la.L2(Op=device_op(la, shape, op), b=y, sigma=SIGMA_F))]:
        smp = la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, n_chains=2, tau=tau, gamma=GAMMA, noise="injected", variant=variant)
        smp.set_state(x0)
        smp.step(1, noise=xi[None])
        got[label] = (smp.get_state().cpu().numpy(), smp.kernel_name)
        smp.close()
    e = R.rel(got["huber"][0], got["plain"][0])
    print(f"delta = inf {shape}: {got['huber'][1]} against {got['plain'][1]}: rel {e:.3e}, bit for bit: {np.array_equal(got['huber'][0], got['plain'][0])}")
    assert "hub" in got["huber"][1] and got["plain"][1] == plain_kernel, (got["huber"][1], got["plain"][1])
    assert R.rel(got["huber"][0], want) < STEP_TOL and R.rel(got["plain"][0], want) < STEP_TOL
    assert e <= 1e-6, e


# ------------------------------------------------------------------ 4. trajectories
@pytest.mark.parametrize("shape", [(20, 33), (24, 264)])
def test_trajectory_matches_reference(la, shape):
    nit = 5
    op, y, d, x0 = case(shape, "blur5")
    ref, pf = R.HuberRef(op, y, d, SIGMA_F), device_term(la, shape, op, y, d)
    R.assert_discriminates(ref, x0, STEP_TOL)
    tau = R.step_size(ref)
    bounds = (0.0, 255.0)
    pg, og = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=bounds), R.TVRef(shape, TV_WEIGHT, 10, bounds)
    C_ = x0.shape[0]
    noise = R.f32(np.random.default_rng(3).standard_normal((nit, C_) + shape))
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    x = x0
    for it in range(nit):
        x = R.myula_step(ref, og, x, tau, GAMMA, noise[it])
        smp.step(1, noise=noise[it:it + 1])
        e = R.rel(smp.get_state().cpu().numpy(), x)
        print(f"trajectory {shape} step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    assert "hub_box" in smp.kernel_name
    smp.close()


# ------------------------------------------------------------------ 5. Philox, sharding
@pytest.mark.parametrize("shape,variant", [((20, 33), "auto"), ((24, 264), "pipe"), ((24, 264), "tile")])
def test_philox_step_is_the_injected_step_with_the_samplers_field(la, shape, variant):
    op, y, d, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, d)
    tau = R.step_size(R.HuberRef(op, y, d, SIGMA_F))
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    kw = dict(n_chains=2, tau=tau, gamma=GAMMA, variant=variant)
    a = la.MYULASampler(pf, pg, shape, seed=7, chain_offset=3, **kw)
    a.set_state(x0)
    field = a.noise_field(0).cpu().numpy()
    a.step(1)
    b = la.MYULASampler(pf, pg, shape, noise="injected", **kw)
    b.set_state(x0)
    b.step(1, noise=field[None])
    ga, gb = a.get_state().cpu().numpy(), b.get_state().cpu().numpy()
    assert "hub" in a.kernel_name and "hub" in b.kernel_name
    a.close()
    b.close()
    assert abs(field.std() - 1.0) < 0.1
    # the same arithmetic on the same field: equal up to the rounding of one fma (two ulps of the largest state) and the 2e-5 per deviate that lmc_device.h
    # states for the device's transcendentals, times sqrt(2 tau)
    assert np.max(np.abs(ga - gb)) <= 2e-5 * np.sqrt(2 * tau) + 2 * np.spacing(np.float32(np.abs(ga).max())), np.max(np.abs(ga - gb))
    assert not np.array_equal(ga, x0.astype(np.float32))


def test_chain_sharding_reproduces_the_trajectories(la):
    """The noise of a chain depends on its global id only: four chains on one sampler are the chains of two samplers of two (chain_offset 0 and 2)."""
    shape = (24, 264)
    op, y, d, x0 = case(shape, "blur5", n_chains=4)
    pf = device_term(la, shape, op, y, d)
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    kw = dict(tau=R.step_size(R.HuberRef(op, y, d, SIGMA_F)), gamma=GAMMA, seed=9)
    whole = la.MYULASampler(pf, pg, shape, n_chains=4, **kw)
    whole.set_state(x0)
    whole.step(3)
    want = whole.get_state().cpu().numpy()
    assert "hub" in whole.kernel_name
    whole.close()
    for off in (0, 2):
        part = la.MYULASampler(pf, pg, shape, n_chains=2, chain_offset=off, **kw)
        part.set_state(x0[off:off + 2])
        part.step(3)
        np.testing.assert_array_equal(part.get_state().cpu().numpy(), want[off:off + 2])
        part.close()


# ------------------------------------------------------------------ 6. SK-ROCK
@pytest.mark.parametrize("shape", [(20, 33), (24, 264)])
def test_skrock_matches_the_restated_recursion(la, shape):
    s, eta, nit = 3, 0.05, 2
    op, y, d, x0 = case(shape, "blur5")
    ref, pf = R.HuberRef(op, y, d, SIGMA_F), device_term(la, shape, op, y, d)
    R.assert_discriminates(ref, x0, STEP_TOL)
    delta = R.step_size(ref)
    pg, og = la.TV(shape, sigma=TV_WEIGHT, niter=10), R.TVRef(shape, TV_WEIGHT, 10)
    Z = R.f32(np.random.default_rng(4).standard_normal((nit,) + x0.shape))
    smp = la.SKROCKSampler(pf, pg, shape, n_stages=s, eta=eta, n_chains=x0.shape[0], tau=delta, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    x = x0
    for it in range(nit):
        x = R.skrock_iteration(ref, og, x, Z[it], delta, GAMMA, s, eta)
        smp.step(1, noise=Z[it:it + 1])
        e = R.rel(smp.get_state().cpu().numpy(), x)
        print(f"SK-ROCK {shape} iteration {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    assert "hub" in smp.kernel_name
    smp.close()


# ------------------------------------------------------------------ 7. SAPG
def test_sapg_runs_on_a_huber_term(la):
    shape, n_updates, seed, C_ = (20, 33), 3, 5, 2
    bounds = (1e-3, 1e2)
    op, y, d, x0 = case(shape, "blur5")
    ref, pf = R.HuberRef(op, y, d, SIGMA_F), device_term(la, shape, op, y, d)
    tau = R.step_size(ref)
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10)
    kw = dict(theta_bounds=bounds, step_scale=0.02, step_exponent=0.8)
    res = la.EstimatePriorWeight(pf, pg, x0, tau, GAMMA, n_updates, bounds, theta0=TV_WEIGHT, step_scale=0.02, step_exponent=0.8, seed=seed, n_chains=C_, dims=shape)
    dim, k = la.sapg_dimension(pg, shape)
    theta, x, trace = TV_WEIGHT, x0, [TV_WEIGHT]
    for n in range(n_updates):
        xi = O.philox_normals(seed, n, np.arange(C_), *shape).astype(np.float64)
        x = R.myula_step(ref, R.TVRef(shape, theta, 10), x, tau, GAMMA, xi)
        gbar = float(np.mean(la.prior_statistic(pg, x, dims=shape).cpu().numpy()))
        theta = la.sapg_update(theta, gbar, n, dim, k, **kw)
        trace.append(theta)
    trace = np.array(trace)
    print(f"SAPG theta trace {res.theta_trace} (reference {trace})")
    assert res.theta_trace.shape == (n_updates + 1,) and res.theta_trace[0] == TV_WEIGHT
    assert np.all((trace[1:] > bounds[0]) & (trace[1:] < bounds[1])) and not np.allclose(trace[1:], TV_WEIGHT), "the updates move theta and none is clamped"
    err = np.abs(res.theta_trace - trace) / trace
    assert np.all(err[1:] < STEP_TOL * np.arange(1, n_updates + 1)), err


# ------------------------------------------------------------------ 8. energies
@pytest.mark.parametrize("data,shape", [("blur5", (20, 33)), ("blur7", (24, 264)), ("identity", (24, 136)), ("nonsep", (20, 33))])
def test_energies_match_reference(la, data, shape):
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, sigma=1.3 * SIGMA_F)
    R.assert_discriminates(ref, x0, STEP_TOL)      # (the plain energy differs from f by more than 100 ENERGY_RTOL)
    pf = device_term(la, shape, op, y, d, sigma=1.3 * SIGMA_F)
    want = ref(x0)
    got = np.asarray(pf(x0))
    assert got.shape == want.shape and np.isfinite(got).all()
    print(f"energies {data} {shape}: HuberLoss.__call__ rel {np.max(np.abs(got - want) / np.abs(want)):.2e}; without -delta^2/2 it would be "
          f"{np.max(np.abs(np.asarray(ref.value_without_offset(x0)) - want) / np.abs(want)):.2e}")
    assert np.max(np.abs(got - want) / np.abs(want)) < ENERGY_RTOL, (got, want)
    assert abs(pf(x0[0]) - want[0]) < ENERGY_RTOL * abs(want[0])
    from lmc_atomi_amd.proximal import _Problem
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    gw = TV_WEIGHT * R.TVRef(shape, 1.0, 1).value(x0)
    f, g = (t.cpu().numpy() for t in _Problem(shape, pf.descriptor(), pg.prior_descriptor()).energies(x0))        # lmc_energies
    assert np.max(np.abs(f - want) / np.abs(want)) < ENERGY_RTOL and np.max(np.abs(g - gw) / gw) < ENERGY_RTOL, (f, want, g, gw)
    smp = la.MYULASampler(pf, pg, shape, n_chains=x0.shape[0], tau=1e-3, gamma=GAMMA)
    smp.set_state(x0)
    f, g = (t.cpu().numpy() for t in smp.energies())                                                              # lmc_sampler_energies
    smp.close()
    assert np.max(np.abs(f - want) / np.abs(want)) < ENERGY_RTOL, (f, want)
    assert np.max(np.abs(g - gw) / gw) < ENERGY_RTOL, (g, gw)


# ------------------------------------------------------------------ 9. MYMALA
MALA_CHAINS, MALA_ITERS, MALA_SEED, MALA_OFFSET = 4, 3, 1234, 40


@pytest.mark.parametrize("shape,kernel", [((20, 33), "myula_step_tile_hub_kernel"), ((24, 264), "myula_step_pipe_hub_kernel")])
def test_mymala_log_alpha_and_states(la, shape, kernel):
    op, y, d, x0 = case(shape, "blur5", n_chains=MALA_CHAINS)
    ref, pf = R.HuberRef(op, y, d, SIGMA_F), device_term(la, shape, op, y, d)
    tau = R.step_size(ref)
    og = R.TVRef(shape, TV_WEIGHT, 10)
    zero = np.zeros((MALA_CHAINS,) + shape)
    mean = lambda v: R.myula_step(ref, og, v, tau, GAMMA, zero)
    g = lambda v: TV_WEIGHT * R.TVRef(shape, 1.0, 1).value(v)
    U = lambda v: np.asarray(ref(v)) + g(v)
    noise = R.f32(np.random.default_rng(6).standard_normal((MALA_ITERS, MALA_CHAINS) + shape))
    uniforms = np.stack([O.philox_uniforms(MALA_SEED, k, MALA_OFFSET + np.arange(MALA_CHAINS)) for k in range(MALA_ITERS)])
    x_ref, acc_ref, la_ref, _, _ = M.mymala(mean, U, x0, tau, noise, uniforms)
    bound = M.bound_of(U(x0))
    safe = (np.abs(np.log(uniforms) - la_ref) > 10 * bound).all(axis=0)
    # on the reference alone: the same chain histories with the PLAIN f in the target give another log alpha, by more than 10 x the bound everywhere
    dec = (np.log(uniforms) <= la_ref).astype(np.int64)
    U_plain = lambda v: np.asarray(ref.plain_value(v)) + g(v)
    la_plain = M.mymala(mean, U_plain, x0, tau, noise, uniforms, decisions=dec)[2]
    print(f"MYMALA {shape}: bound {bound:.3e}; log alpha {la_ref.tolist()}; with the plain f it moves by {np.abs(la_plain - la_ref).min():.3e} at the least; "
          f"safe chains {int(safe.sum())}/{MALA_CHAINS}")
    assert (np.abs(la_plain - la_ref) > 10 * bound).all(), (la_plain, la_ref, bound)
    smp = la.MYMALASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, n_chains=MALA_CHAINS, tau=tau, gamma=GAMMA, noise="injected", seed=MALA_SEED,
                           chain_offset=MALA_OFFSET)
    try:
        smp.set_state(x0.copy())
        las, accs = [], []
        for k in range(MALA_ITERS):
            smp.step(1, noise=noise[k:k + 1].copy())
            acc, la_d = smp.acceptance()
            las.append(la_d.cpu().numpy())
            accs.append(acc.cpu().numpy())
        got, name = smp.get_state().cpu().numpy(), smp.kernel_name
    finally:
        smp.close()
    assert name == kernel, name
    dec_d = np.diff(np.array([np.zeros_like(accs[0])] + accs), axis=0)
    if (dec_d != dec)[:, ~safe].any():     # a borderline decision went the other way: the reference follows the device on the chains that have one
        x_ref, acc_ref, la_ref, _, _ = M.mymala(mean, U, x0, tau, noise, uniforms, decisions=np.where(safe[None, :], -1, dec_d))
        dec = np.where(safe[None, :], dec, dec_d)
    agree = np.vstack([np.ones((1, MALA_CHAINS), dtype=bool), np.cumprod(dec_d == dec, axis=0).astype(bool)[:-1]])
    err = np.abs(np.array(las) - la_ref)
    print(f"MYMALA {shape}: {name}; max |log alpha error| / bound {(err / bound)[agree].max():.3f}; accepted {accs[-1].tolist()} (reference {acc_ref.tolist()})")
    assert (err[agree] < bound).all(), (las, la_ref, bound)
    assert (accs[-1][safe] == acc_ref[safe]).all(), (accs[-1], acc_ref, safe)
    if safe.any():
        assert R.rel(got[safe], x_ref[safe]) < STATE_TOL


# ------------------------------------------------------------------ 10. moments, histograms, groups through the functional interface
def test_functional_interface_and_diagnostics_take_a_huber_term(la):
    shape = (24, 264)
    op, y, d, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, d)
    tau = R.step_size(R.HuberRef(op, y, d, SIGMA_F))
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0[0].ravel(), tau=tau, gamma=GAMMA, niter=6, seed=3, n_chains=4, dims=shape,
                                            moment_scales=(2,), hist_bins=8, hist_range=(0.0, 255.0), chain_groups=2,
                                            cov_probes=la.random_probes(3, shape, seed=1))
    mean = np.asarray(res.mean.cpu() if hasattr(res.mean, "cpu") else res.mean)
    assert res.count > 0 and np.isfinite(mean).all()
    res = la.StabilisedLangevin(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), x0[0].ravel(), tau=tau, gamma=GAMMA, niter=3, n_stages=3, n_chains=2, dims=shape)
    assert res.count > 0
    res = la.MoreauYosidaMetropolisAdjustedLangevin(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), x0[0].ravel(), tau=tau, gamma=GAMMA, niter=2, n_chains=2, dims=shape)
    assert res is not None


# ------------------------------------------------------------------ 11. the large PSF: one general and one separable kernel, the smallest with several tiles
PSF_NAMES = ["gen-33x65-17x17", "sep-37x70-33x15"]


@functools.lru_cache(maxsize=None)
def psf_case(name):
    c = PS.CASES[PS.IDS.index(name)]
    op = R.Op("blur", c.h.astype(np.float64), c.offset)
    _, op, y, d, x0 = R.recipe(c.shape, n_chains=2, op=op)
    for a in (y, d, x0):
        a.setflags(write=False)
    return c, op, y, d, x0


@pytest.mark.parametrize("name", PSF_NAMES)
def test_large_psf_gradient_step_and_energy(la, name):
    c, op, y, d, x0 = psf_case(name)
    shape = c.shape
    assert (shape[0] + 31) // 32 * ((shape[1] + 63) // 64) > 1 and min(c.h.shape) > 9       # several 32 x 64 tiles; beyond LMC_MAX_BLUR
    ref = R.HuberRef(op, y, d, SIGMA_F)
    R.assert_discriminates(ref, x0, STEP_TOL)
    dop = la.PSF(shape, c.h, offset=c.offset)
    assert (dop.factors is not None) == c.separable
    pf = la.HuberLoss(dop, y, d, sigma=SIGMA_F)
    r32 = R.HuberRef(R.Op("blur", c.h, c.offset), y, d, SIGMA_F, dtype=np.float32)
    got = pf.grad(x0)
    want = ref.grad(x0)
    e = R.rel(got, want)
    print(f"PSF {name}: gradient rel {e:.3e}")
    assert e < STEP_TOL, e
    per_pixel(f"PSF grad {name}", got, want, r32.grad(x0.astype(np.float32)))
    tau = R.step_size(ref)
    bounds = (0.0, 255.0)
    pg, og = priors(la, shape, "tv", bounds)
    xi = R.f32(np.random.default_rng(8).standard_normal(x0.shape))
    want = R.myula_step(ref, og, x0, tau, GAMMA, xi)
    smp = la.MYULASampler(pf, pg, shape, n_chains=2, tau=tau, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    smp.step(1, noise=xi[None])
    got = smp.get_state().cpu().numpy()
    f, _ = (t.cpu().numpy() for t in smp.energies())
    smp.close()
    e = R.rel(got, want)
    print(f"PSF {name}: step rel {e:.3e}")
    assert e < STEP_TOL, e
    per_pixel(f"PSF step {name}", got, want, R.myula_step(r32, priors(la, shape, "tv", bounds, dtype=np.float32)[1], x0, tau, GAMMA, xi, dtype=np.float32))
    fw = np.asarray(ref(got.astype(np.float64)))
    assert np.max(np.abs(f - fw) / np.abs(fw)) < ENERGY_RTOL, (f, fw)
    fx = np.asarray(pf(x0))
    assert np.max(np.abs(fx - np.asarray(ref(x0))) / np.abs(np.asarray(ref(x0)))) < ENERGY_RTOL, (fx, ref(x0))
    with pytest.raises(NotImplementedError):
        la.MYMALASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, n_chains=2, tau=tau, gamma=GAMMA)


# ------------------------------------------------------------------ 12. refusals
def myula_config(la, shape, data, prior, **fields):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    prob = _Problem(shape, data, prior)
    for k, v in fields.items():
        setattr(prob.c, k, v)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = 2
    cfg.tau, cfg.gamma, cfg.epsg = 1e-3, GAMMA, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return prob, cfg


def last_error():
    from lmc_atomi_amd import _dev
    return _dev.lib().lmc_last_error().decode()


REFUSED = [dict(ncvx_kind=1, ncvx_gamma=1.0), dict(tv_rtol=1e-4), dict(tv_warm=1, tv_niter=3), dict(prior_kind=5), dict(step_variant=3), dict(step_variant=6),
           dict(step_variant=8), dict(step_variant=7)]      # 7 on a 24 x 96 image: not covered


@pytest.mark.parametrize("data", ["blur5", "identity"])
def test_c_abi_refusals(la, data):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    shape = (24, 96)
    op, y, d, x0 = case(shape, data)
    pf = device_term(la, shape, op, y, d)
    prior = la.TV(shape, sigma=TV_WEIGHT, niter=10).prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    for fields in REFUSED:
        prob, cfg = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert prob.c.data_kind in _capi.HUBER_KINDS
        for create in (lambda h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_mymala_create(C.byref(cfg), C.byref(h)),
                       lambda h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h))):
            hnd = C.c_void_p()
            rc = create(hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == LMC_E_UNSUPPORTED and msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, _dev.stream_ptr(x.device))
        assert rc == LMC_E_UNSUPPORTED and last_error(), (fields, rc, last_error())
    # the sampler and the entry point without a Huber form
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "Huber" in last_error() and not hnd.value, (rc, last_error())
    ws = torch.empty(lib.lmc_l2_prox_workspace_bytes(2, *shape), dtype=torch.uint8, device="cuda")
    rc = lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 5, 0, _dev.ptr(ws), _dev.stream_ptr(x.device))
    assert rc == LMC_E_UNSUPPORTED and "Huber" in last_error(), (rc, last_error())
    # a mask with the term is LMC_E_INVALID: there is no Huber mask kind
    prob_m, cfg_m = myula_config(la, shape, pf.descriptor(), prior, mask_dev=_dev.ptr(x))
    assert lib.lmc_myula_create(C.byref(cfg_m), C.byref(hnd)) == LMC_E_INVALID and "mask" in last_error() and not hnd.value
    # MYMALA's other refusals stand: a box on the prior
    prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0)).prior_descriptor())
    rc = lib.lmc_mymala_create(C.byref(cfg_b), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and last_error() and not hnd.value, (rc, last_error())
    # kind 16 is no kind
    prob16, cfg16 = myula_config(la, shape, pf.descriptor(), prior, data_kind=16)
    assert lib.lmc_myula_create(C.byref(cfg16), C.byref(hnd)) == LMC_E_INVALID and not hnd.value
    # what is not refused: the problem as it stands, by MYULA and by MYMALA
    for create in (lib.lmc_myula_create, lib.lmc_mymala_create):
        assert create(C.byref(cfg), C.byref(hnd)) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
    torch.cuda.synchronize()


def test_c_abi_mymala_refuses_the_psf_kind(la):
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    c, op, y, d, x0 = psf_case(PSF_NAMES[0])
    pf = la.HuberLoss(la.PSF(c.shape, c.h, offset=c.offset), y, d, sigma=SIGMA_F)
    prob, cfg = myula_config(la, c.shape, pf.descriptor(), la.TV(c.shape, sigma=TV_WEIGHT, niter=10).prior_descriptor())
    assert prob.c.data_kind == _capi.DATA_HUBER_PSF
    hnd = C.c_void_p()
    rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "PSF" in last_error() and not hnd.value, (rc, last_error())
    assert lib.lmc_myula_create(C.byref(cfg), C.byref(hnd)) == 0, last_error()
    lib.lmc_sampler_destroy(hnd)


def test_python_refusals(la):
    shape = (24, 96)
    op, y, d, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, d)
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10)
    kw = dict(n_chains=2, tau=1e-3, gamma=GAMMA)
    with pytest.raises(NotImplementedError):
        la.UnadjustedLangevinPrimalDual(pf, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), x0[0].ravel(), tau=0.1, mu=0.1, niter=2)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10, rtol=1e-4), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=3, warm=True), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=3), shape, tv_warm=True, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.WaveletL1(shape, sigma=0.3), shape, **kw)
    for variant in ("split", "point", "block", "rows", "pipe2"):
        with pytest.raises(NotImplementedError):
            la.MYULASampler(pf, pg, shape, variant=variant, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, pg, shape, variant="pipe", **kw)          # 96 columns: the pipeline does not cover it
    with pytest.raises(NotImplementedError):
        la.SKROCKSampler(pf, pg, shape, n_stages=3, variant="rows", **kw)
    with pytest.raises(NotImplementedError):
        la.MYMALASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0)), shape, **kw)      # MYMALA's own refusals stand
    with pytest.raises(NotImplementedError):
        pf.prox(x0[0], 1.0)
    la.MYULASampler(pf, pg, shape, **kw).close()
    la.MYMALASampler(pf, pg, shape, **kw).close()
