"""GPU parity of the weighted Gaussian data term (LMC_DATA_WL2_* in include/lmc_atomi.h, `la.L2(weights=...)`) against the float64 reference of
tests/_wl2_ref.py: the gradient through `lmc_fused_eval`, the fused MYULA step in the tiled kernel (`myula_step_tile_wl2_kernel` /
`myula_step_tile_wl2_box_kernel`) and in the full-width pipeline (`myula_step_pipe_wl2_kernel` / `myula_step_pipe_wl2_box_kernel`), what falls back to
the tiled kernel, weights = 1 against the unweighted term, trajectories, the Philox path, chain sharding, SK-ROCK, SAPG, the energies, MYMALA's
Metropolis ratio, and the refusals of the C ABI and of the Python surface.

Tolerances are the project's: one operator or one step rel-L2 <= 1e-5, 1e-5 x (step index) along a trajectory, energies rtol 5e-5
(tests/test_gpu_poisson.py); MYMALA: log alpha within 2e-6 max|U(x0)| + 2e-3, states rel-L2 2e-5 on the clear-cut chains
(tests/test_gpu_mymala_matrix.py).  Every comparison is against `WL2Ref`, never against another device path, except the one test that says so.  Every
case first asserts, on the reference alone (`R.assert_discriminates`), that >= 10 % of the pixels have w = 0 and that a kernel which ignores the weights
or multiplies by them after the adjoint would miss the tolerance thirty- to a hundredfold."""
import ctypes as C
import functools

import numpy as np
import pytest

import _wl2_ref as R
from oracle import lmc_oracle as O
from tests import _mala_ref as M

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-5
ENERGY_RTOL = 5e-5
STATE_TOL = 2e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2
INF = R.INF
GAMMA, TV_WEIGHT, SIGMA_F = R.GAMMA, R.TV_WEIGHT, R.SIGMA_F
NONSEP = (np.array([[0.05, 0.2, 0.0], [0.1, 0.3, 0.15], [0.0, 0.05, 0.15]]), (0, 2))       # off-centre origin: not a centred separable blur


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


@functools.lru_cache(maxsize=None)
def case(shape, data="blur5", n_chains=2, edge=False):
    """(reference operator, y, w, x0) of one configuration, computed once; read-only.  `edge`: weights 0 on the whole last column and last row."""
    if data.startswith("blur"):
        op = R.Op("blur", *R.box_kernel(int(data[4:])))
    elif data == "nonsep":
        op = R.Op("blur", *NONSEP)
    else:
        op = R.Op("identity")
    _, op, y, w, x0 = R.recipe(shape, n_chains=n_chains, op=op)
    if edge:
        w[:, -1] = 0.0
        w[-1, :] = 0.0
    for a in (y, w, x0):
        a.setflags(write=False)
    return op, y, w, x0


def device_op(la, shape, op):
    return la.Convolve2D(shape, op.args[0], offset=op.args[1]) if op.kind == "blur" else la.Identity(shape[0] * shape[1])


def device_term(la, shape, op, y, w, sigma=SIGMA_F):
    return la.L2(Op=device_op(la, shape, op), b=y, sigma=sigma, weights=w, dims=shape)


def priors(la, shape, prior, bounds, niter=10, iso=True):
    if prior == "tv":
        return la.TV(shape, sigma=TV_WEIGHT, niter=niter, isotropic=iso, bounds=bounds), R.TVRef(shape, TV_WEIGHT, niter, bounds, aniso=not iso)
    if prior == "l1":
        return la.L1(sigma=0.2, bounds=bounds), R.SeparableRef(lambda v, t: O.L1(0.2).prox(v, t), bounds)
    if prior == "l2":
        return la.L2(sigma=0.05, dims=shape, bounds=bounds), R.SeparableRef(lambda v, t: v / (1.0 + t * 0.05), bounds)
    if prior == "laplace":
        return la.Laplace(0.2, bounds=bounds), R.SeparableRef(lambda v, t: O.prox_laplace(v, t * 0.2), bounds)
    raise ValueError(prior)


# ------------------------------------------------------------------ 1. gradient
GRAD_CASES = [("blur5", (20, 33)), ("blur7", (20, 33)), ("blur5", (37, 150)), ("blur7", (37, 150)), ("nonsep", (20, 33)), ("identity", (20, 33))]


@pytest.mark.parametrize("data,shape", GRAD_CASES)
def test_gradient_matches_reference(la, data, shape):
    op, y, w, x0 = case(shape, data)
    ref = R.WL2Ref(op, y, w, sigma=1.3 * SIGMA_F)
    stats = R.assert_discriminates(ref, x0, STEP_TOL)
    pf = device_term(la, shape, op, y, w, sigma=1.3 * SIGMA_F)
    got = pf.grad(x0)
    assert got.shape == x0.shape
    e = R.rel(got, ref.grad(x0))
    print(f"grad {data} {shape}: rel {e:.3e}; w=0 {stats[0]:.2f}, unweighted {stats[1]:.2e}, post-adjoint {stats[2]}")
    assert e < STEP_TOL, e
    assert R.rel(pf.grad(x0[0].ravel()), ref.grad(x0[0]).ravel()) < STEP_TOL       # a flat image in, a flat gradient out


# ------------------------------------------------------------------ 2. one MYULA step, injected noise
def one_step(la, shape, data, bounds, variant, niter=10, iso=True, prior="tv", edge=False):
    """-> (rel-L2 of one injected-noise MYULA step against the reference, kernel name); asserts that the comparison discriminates."""
    op, y, w, x0 = case(shape, data, edge=edge)
    ref = R.WL2Ref(op, y, w, SIGMA_F)
    R.assert_discriminates(ref, x0, STEP_TOL)
    pf = device_term(la, shape, op, y, w)
    tau = R.step_size(ref)
    assert pf.grad_lipschitz() == pytest.approx(ref.grad_lipschitz(), rel=1e-6)      # (the operator keeps its taps in fp32: 6e-8 each, squared)
    pg, og = priors(la, shape, prior, bounds, niter, iso)
    xi = np.random.default_rng(shape[1]).standard_normal(x0.shape)
    want = R.myula_step(ref, og, x0, tau, GAMMA, xi)
    smp = la.MYULASampler(pf, pg, shape, n_chains=x0.shape[0], tau=tau, gamma=GAMMA, noise="injected", variant=variant)
    smp.set_state(x0)
    smp.step(1, noise=xi[None])
    got = smp.get_state().cpu().numpy()
    name = smp.kernel_name
    smp.close()
    assert np.isfinite(got).all(), "NaN / inf in the state (masking of lanes past the row end?)"
    return R.rel(got, want), name


@pytest.mark.parametrize("bounds", R.BOXES, ids=["free", "positive", "box"])
@pytest.mark.parametrize("data,shape", [("blur5", (20, 33)), ("blur5", (40, 128)), ("identity", (20, 33)), ("nonsep", (20, 33))])
def test_myula_step_tile(la, data, shape, bounds):
    e, name = one_step(la, shape, data, bounds, "auto")
    print(f"tile {data} {shape} bounds={bounds}: rel {e:.3e} ({name})")
    assert name == ("myula_step_tile_wl2_box_kernel" if bounds else "myula_step_tile_wl2_kernel"), name
    assert e < STEP_TOL, e


@pytest.mark.parametrize("shape,kw", [((24, 264), dict(iso=False)), ((24, 136), dict(niter=20)), ((24, 264), dict(niter=9)),
                                      ((24, 136), dict(prior="l1")), ((24, 264), dict(prior="l2")), ((24, 136), dict(prior="laplace"))],
                         ids=["aniso", "K20", "K9", "l1", "l2", "laplace"])
def test_fallbacks_run_the_tile_kernel(la, shape, kw):
    for bounds in (None, (0.0, 255.0)):
        e, name = one_step(la, shape, "blur5", bounds, "auto", **kw)
        print(f"fallback {kw} {shape} bounds={bounds}: rel {e:.3e} ({name})")
        assert name.startswith("myula_step_tile_wl2"), name
        assert e < STEP_TOL, e


# shape -> what it reaches: PXL 4 aligned / lanes past the row end, PXL 8 aligned / past the row end, two strips
PIPE_CASES = [("blur5", (24, 136)), ("blur5", (24, 150)), ("blur5", (24, 264)), ("blur5", (24, 268)), ("blur5", (16, 520)), ("blur7", (24, 264)),
              ("identity", (24, 136))]


@pytest.mark.parametrize("bounds", R.BOXES, ids=["free", "positive", "box"])
@pytest.mark.parametrize("data,shape", PIPE_CASES)
def test_myula_step_pipe(la, data, shape, bounds):
    e, name = one_step(la, shape, data, bounds, "pipe")
    print(f"pipe {data} {shape} bounds={bounds}: rel {e:.3e} ({name})")
    assert name == ("myula_step_pipe_wl2_box_kernel" if bounds else "myula_step_pipe_wl2_kernel"), name
    assert e < STEP_TOL, e


def test_myula_step_pipe_with_an_unobserved_last_column_and_row(la):
    """Weights 0 on the whole last image column and last row at 24 x 150, where the last lanes reach past the row end."""
    e, name = one_step(la, (24, 150), "blur5", (0.0, 255.0), "pipe", edge=True)
    print(f"pipe edge weights: rel {e:.3e} ({name})")
    assert name == "myula_step_pipe_wl2_box_kernel" and e < STEP_TOL, (name, e)


AUTO_KERNEL_24x264 = "myula_step_pipe_wl2_box_kernel"      # DESIGN "Weighted Gaussian data term": the measured step times decide what auto picks


def test_tile_pipe_and_auto_agree_with_the_reference(la):
    e1, n1 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "tile")
    e7, n7 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "pipe")
    e0, n0 = one_step(la, (24, 264), "blur5", (0.0, 255.0), "auto")
    print(f"24 x 264: tile {e1:.3e} ({n1}), pipe {e7:.3e} ({n7}), auto {e0:.3e} ({n0})")
    assert n1 == "myula_step_tile_wl2_box_kernel" and n7 == "myula_step_pipe_wl2_box_kernel"
    assert max(e1, e7, e0) < STEP_TOL
    assert n0 == AUTO_KERNEL_24x264, n0


def test_forced_pipe_on_an_uncovered_problem_raises(la):
    shape = (20, 33)
    op, y, w, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, w)
    kw = dict(n_chains=2, tau=1e-3, gamma=GAMMA, variant="pipe")
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, **kw)            # 33 columns
    shape = (24, 264)
    op, y, w, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, w)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10, isotropic=False), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=9), shape, **kw)


def test_lagged_output_of_eleven_is_ten_and_runs_the_pipe(la):
    shape = (24, 264)
    op, y, w, x0 = case(shape, "blur5")
    ref, pf = R.WL2Ref(op, y, w, SIGMA_F), device_term(la, shape, op, y, w)
    tau = R.step_size(ref)
    xi = np.random.default_rng(1).standard_normal(x0.shape)
    smp = la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=11, lagged_output=True), shape, n_chains=2, tau=tau, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    smp.step(1, noise=xi[None])
    e = R.rel(smp.get_state().cpu().numpy(), R.myula_step(ref, R.TVRef(shape, TV_WEIGHT, 10), x0, tau, GAMMA, xi))
    assert smp.kernel_name == "myula_step_pipe_wl2_kernel" and e < STEP_TOL, (smp.kernel_name, e)
    smp.close()


# ------------------------------------------------------------------ 3. weights = 1 is the unweighted term (device against device: the one place)
@pytest.mark.parametrize("shape", [(20, 33), (24, 264)])
def test_unit_weights_are_the_unweighted_term(la, shape):
    op, y, _, x0 = case(shape, "blur5")
    ones = np.ones(shape)
    ref = R.WL2Ref(op, y, ones, SIGMA_F)
    tau = R.step_size(ref)
    xi = np.random.default_rng(2).standard_normal(x0.shape)
    want = R.myula_step(ref, R.TVRef(shape, TV_WEIGHT, 10), x0, tau, GAMMA, xi)
    got = {}
    for label, pf in [("weighted", device_term(la, shape, op, y, ones)), ("plain", la.L2(Op=device_op(la, shape, op), b=y, sigma=SIGMA_F))]:
        smp = la.MYULASampler(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), shape, n_chains=2, tau=tau, gamma=GAMMA, noise="injected")
        smp.set_state(x0)
        smp.step(1, noise=xi[None])
        got[label] = (smp.get_state().cpu().numpy(), smp.kernel_name)
        smp.close()
    print(f"unit weights {shape}: {got['weighted'][1]} against {got['plain'][1]}: rel {R.rel(got['weighted'][0], got['plain'][0]):.3e}")
    assert "wl2" in got["weighted"][1] and "wl2" not in got["plain"][1]
    assert R.rel(got["weighted"][0], want) < STEP_TOL and R.rel(got["plain"][0], want) < STEP_TOL
    assert R.rel(got["weighted"][0], got["plain"][0]) < STEP_TOL


# ------------------------------------------------------------------ 4. trajectories
@pytest.mark.parametrize("shape", [(20, 33), (24, 264)])
def test_trajectory_matches_reference(la, shape):
    nit = 5
    op, y, w, x0 = case(shape, "blur5")
    ref, pf = R.WL2Ref(op, y, w, SIGMA_F), device_term(la, shape, op, y, w)
    R.assert_discriminates(ref, x0, STEP_TOL)
    tau = R.step_size(ref)
    bounds = (0.0, 255.0)
    pg, og = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=bounds), R.TVRef(shape, TV_WEIGHT, 10, bounds)
    C_ = x0.shape[0]
    noise = np.random.default_rng(3).standard_normal((nit, C_) + shape)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C_, tau=tau, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    x = x0
    for it in range(nit):
        x = R.myula_step(ref, og, x, tau, GAMMA, noise[it])
        smp.step(1, noise=noise[it:it + 1])
        e = R.rel(smp.get_state().cpu().numpy(), x)
        print(f"trajectory {shape} step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    assert "wl2_box" in smp.kernel_name
    smp.close()


# ------------------------------------------------------------------ 5. Philox, sharding
@pytest.mark.parametrize("shape,variant", [((20, 33), "auto"), ((24, 264), "pipe"), ((24, 264), "tile")])
def test_philox_step_is_the_injected_step_with_the_samplers_field(la, shape, variant):
    op, y, w, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, w)
    tau = R.step_size(R.WL2Ref(op, y, w, SIGMA_F))
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
    op, y, w, x0 = case(shape, "blur5", n_chains=4)
    pf = device_term(la, shape, op, y, w)
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    kw = dict(tau=R.step_size(R.WL2Ref(op, y, w, SIGMA_F)), gamma=GAMMA, seed=9)
    whole = la.MYULASampler(pf, pg, shape, n_chains=4, **kw)
    whole.set_state(x0)
    whole.step(3)
    want = whole.get_state().cpu().numpy()
    assert "wl2" in whole.kernel_name
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
    op, y, w, x0 = case(shape, "blur5")
    ref, pf = R.WL2Ref(op, y, w, SIGMA_F), device_term(la, shape, op, y, w)
    R.assert_discriminates(ref, x0, STEP_TOL)
    delta = R.step_size(ref)
    pg, og = la.TV(shape, sigma=TV_WEIGHT, niter=10), R.TVRef(shape, TV_WEIGHT, 10)
    Z = np.random.default_rng(4).standard_normal((nit,) + x0.shape)
    smp = la.SKROCKSampler(pf, pg, shape, n_stages=s, eta=eta, n_chains=x0.shape[0], tau=delta, gamma=GAMMA, noise="injected")
    smp.set_state(x0)
    x = x0
    for it in range(nit):
        x = R.skrock_iteration(ref, og, x, Z[it], delta, GAMMA, s, eta)
        smp.step(1, noise=Z[it:it + 1])
        e = R.rel(smp.get_state().cpu().numpy(), x)
        print(f"SK-ROCK {shape} iteration {it + 1}: rel {e:.3e} ({smp.kernel_name})")
        assert e < STEP_TOL * (it + 1), (it, e)
    assert "wl2" in smp.kernel_name
    smp.close()


# ------------------------------------------------------------------ 7. SAPG
def test_sapg_runs_on_a_weighted_term(la):
    shape, n_updates, seed, C_ = (20, 33), 3, 5, 2
    bounds = (1e-3, 1e2)
    op, y, w, x0 = case(shape, "blur5")
    ref, pf = R.WL2Ref(op, y, w, SIGMA_F), device_term(la, shape, op, y, w)
    tau = R.step_size(ref)
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10)
    kw = dict(theta_bounds=bounds, step_scale=0.02, step_exponent=0.8)
    res = la.EstimatePriorWeight(pf, pg, x0, tau, GAMMA, n_updates, bounds, theta0=TV_WEIGHT, step_scale=0.02, step_exponent=0.8, seed=seed, n_chains=C_, dims=shape)
    d, k = la.sapg_dimension(pg, shape)
    theta, x, trace = TV_WEIGHT, x0, [TV_WEIGHT]
    for n in range(n_updates):
        xi = O.philox_normals(seed, n, np.arange(C_), *shape).astype(np.float64)
        x = R.myula_step(ref, R.TVRef(shape, theta, 10), x, tau, GAMMA, xi)
        gbar = float(np.mean(la.prior_statistic(pg, x, dims=shape).cpu().numpy()))
        theta = la.sapg_update(theta, gbar, n, d, k, **kw)
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
    op, y, w, x0 = case(shape, data)
    ref = R.WL2Ref(op, y, w, sigma=1.3 * SIGMA_F)
    R.assert_discriminates(ref, x0, STEP_TOL)      # (the unweighted energy differs from f by more than 100 ENERGY_RTOL)
    pf = device_term(la, shape, op, y, w, sigma=1.3 * SIGMA_F)
    want = ref(x0)
    got = np.asarray(pf(x0))
    assert got.shape == want.shape
    print(f"energies {data} {shape}: L2.__call__ rel {np.max(np.abs(got - want) / np.abs(want)):.2e}")
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
MALA_STATE_NOISE = 10.0      # the recipe's: at it the unweighted f moves log alpha by more than 10 x the bound on every chain (asserted below)


@pytest.mark.parametrize("shape,kernel", [((20, 33), "myula_step_tile_wl2_kernel"), ((24, 264), "myula_step_pipe_wl2_kernel")])
def test_mymala_log_alpha_and_states(la, shape, kernel):
    op, y, w, x0 = case(shape, "blur5", n_chains=MALA_CHAINS)
    ref, pf = R.WL2Ref(op, y, w, SIGMA_F), device_term(la, shape, op, y, w)
    tau = R.step_size(ref)
    og = R.TVRef(shape, TV_WEIGHT, 10)
    zero = np.zeros((MALA_CHAINS,) + shape)
    mean = lambda v: R.myula_step(ref, og, v, tau, GAMMA, zero)
    g = lambda v: TV_WEIGHT * R.TVRef(shape, 1.0, 1).value(v)
    U = lambda v: np.asarray(ref(v)) + g(v)
    noise = np.random.default_rng(6).standard_normal((MALA_ITERS, MALA_CHAINS) + shape)
    uniforms = np.stack([O.philox_uniforms(MALA_SEED, k, MALA_OFFSET + np.arange(MALA_CHAINS)) for k in range(MALA_ITERS)])
    x_ref, acc_ref, la_ref, _, _ = M.mymala(mean, U, x0, tau, noise, uniforms)
    bound = M.bound_of(U(x0))
    safe = (np.abs(np.log(uniforms) - la_ref) > 10 * bound).all(axis=0)
    # on the reference alone: the same chain histories with the UNWEIGHTED f in the target give another log alpha, by more than 10 x the bound everywhere
    dec = (np.log(uniforms) <= la_ref).astype(np.int64)
    U_unw = lambda v: np.asarray(ref.unweighted_value(v)) + g(v)
    la_unw = M.mymala(mean, U_unw, x0, tau, noise, uniforms, decisions=dec)[2]
    print(f"MYMALA {shape}: bound {bound:.3e}; log alpha {la_ref.tolist()}; with the unweighted f it moves by {np.abs(la_unw - la_ref).min():.3e} at the least; "
          f"safe chains {int(safe.sum())}/{MALA_CHAINS}")
    assert (np.abs(la_unw - la_ref) > 10 * bound).all(), (la_unw, la_ref, bound)
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
def test_functional_interface_and_diagnostics_take_a_weighted_term(la):
    shape = (24, 264)
    op, y, w, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, w)
    tau = R.step_size(R.WL2Ref(op, y, w, SIGMA_F))
    pg = la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0))
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, x0[0].ravel(), tau=tau, gamma=GAMMA, niter=6, seed=3, n_chains=4, dims=shape,
                                            moment_scales=(2,), hist_bins=8, hist_range=(0.0, 255.0), chain_groups=2)
    mean = np.asarray(res.mean.cpu() if hasattr(res.mean, "cpu") else res.mean)
    assert res.count > 0 and np.isfinite(mean).all()
    res = la.StabilisedLangevin(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), x0[0].ravel(), tau=tau, gamma=GAMMA, niter=3, n_stages=3, n_chains=2, dims=shape)
    assert res.count > 0
    res = la.MoreauYosidaMetropolisAdjustedLangevin(pf, la.TV(shape, sigma=TV_WEIGHT, niter=10), x0[0].ravel(), tau=tau, gamma=GAMMA, niter=2, n_chains=2, dims=shape)
    assert res is not None


# ------------------------------------------------------------------ 11. refusals
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
    op, y, w, x0 = case(shape, data)
    pf = device_term(la, shape, op, y, w)
    prior = la.TV(shape, sigma=TV_WEIGHT, niter=10).prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    for fields in REFUSED:
        prob, cfg = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert prob.c.data_kind in _capi.WL2_KINDS
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
    # the sampler and the entry point without a weighted form
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "weighted" in last_error() and not hnd.value, (rc, last_error())
    ws = torch.empty(lib.lmc_l2_prox_workspace_bytes(2, *shape), dtype=torch.uint8, device="cuda")
    rc = lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 5, 0, _dev.ptr(ws), _dev.stream_ptr(x.device))
    assert rc == LMC_E_UNSUPPORTED and "weighted" in last_error(), (rc, last_error())
    # MYMALA's other refusals stand: a box on the prior
    prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), la.TV(shape, sigma=TV_WEIGHT, niter=10, bounds=(0.0, 255.0)).prior_descriptor())
    rc = lib.lmc_mymala_create(C.byref(cfg_b), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and last_error() and not hnd.value, (rc, last_error())
    # kind 9 is no kind
    prob9, cfg9 = myula_config(la, shape, pf.descriptor(), prior, data_kind=9)
    assert lib.lmc_myula_create(C.byref(cfg9), C.byref(hnd)) == LMC_E_INVALID and not hnd.value
    # what is not refused: the problem as it stands, by MYULA and by MYMALA
    for create in (lib.lmc_myula_create, lib.lmc_mymala_create):
        assert create(C.byref(cfg), C.byref(hnd)) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
    torch.cuda.synchronize()


def test_python_refusals(la):
    shape = (24, 96)
    op, y, w, x0 = case(shape, "blur5")
    pf = device_term(la, shape, op, y, w)
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
