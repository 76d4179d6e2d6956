"""GPU parity of the Fourier-domain data term (`la.FourierSampling`, `la.PeriodicConvolve2D`, `la.rfft2` / `la.irfft2`; LMC_DATA_SPECTRAL in
include/lmc_atomi.h) against the references of tests/_fourier_ref.py: the transforms per bin and pixel, the periodic blur and its adjoint against the
direct wrap-around sum, more than 65535 images, one MYULA step per pixel for the priors that take another kernel in the prior launch, the closed-form
prox, the Philox path, chain sharding, SK-ROCK, SAPG, the energies, and the refusals of the C ABI and of the Python surface.

Per pixel / bin: max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|)) over every chain and pixel, e32 measured on numpy's single-precision replay
(tests/_pixel.py's bound).  Trajectories: the project's rel-L2 1e-5 x (step index); energies: rtol 5e-5."""
import ctypes as C

import numpy as np
import pytest

import _fourier_ref as F
import _many as M
import _pixel as X
import _poisson_ref as P
from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-5
ENERGY_RTOL = 5e-5
LMC_E_INVALID, LMC_E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


def within(what, got, ref64, bound, e32):
    err, where = F.worst(got, ref64)
    print(f"pixel {what}: err {err:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert err <= bound, (what, err, bound, where)
    return err


# ------------------------------------------------------------------ 1. the transforms
@pytest.mark.parametrize("shape", F.SHAPES, ids=F.SHAPE_IDS)
def test_transforms_per_bin_and_pixel(la, shape):
    fw, inv, rt = F.rfft2_reference(shape), F.irfft2_reference(shape), F.roundtrip_reference(shape)
    got = la.rfft2(fw.x)
    assert got.shape == fw.x.shape[:-1] + (shape[1] // 2 + 1,) and got.dtype == np.complex64
    within(f"rfft2 {shape}", F.ri(got), fw.ref64, fw.bound, fw.e32)
    back = la.irfft2(inv.x, shape)
    assert back.shape == inv.x.shape[:-2] + shape and back.dtype == np.float32
    within(f"irfft2 {shape}", back, inv.ref64, inv.bound, inv.e32)
    within(f"round trip {shape}", la.irfft2(got, shape), rt.ref64, rt.bound, rt.e32)
    one = la.rfft2(fw.x[1])                       # a single image, no batch axis
    within(f"rfft2 {shape} one image", F.ri(one)[None], fw.ref64[1:2], fw.bound, fw.e32)


def test_more_images_than_a_grid_dimension_holds(la):
    """70000 images of 8 x 8: image c is pattern c % 7, so an image index that wraps or loses its chunk shows as another pattern."""
    import torch
    n, shape = 70000, (8, 8)
    base = M.patterns(shape, seed=4)
    base = X.f32(base - base.mean(axis=(-2, -1), keepdims=True))
    x = M.tile_dev(base, n)
    r64 = F.ri(np.fft.rfft2(base.astype(np.float64), norm="ortho"))
    e32, bound = X.bound_of(r64, F.ri(np.fft.rfft2(base, norm="ortho")))
    spec = la.rfft2(x)
    got = torch.view_as_real(spec).cpu().numpy()
    assert got.shape == (n, 8, 5, 2)
    d = np.abs(got.astype(np.float64) - r64[M.tile_index(n)])
    d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    print(f"70000 images rfft2: err {d[k]:.3e} at image {k[0]} (pattern {k[0] % M.P}), bound {bound:.3e}")
    assert d[k] <= bound, (k, d[k], bound)
    back = la.irfft2(spec, shape).cpu().numpy()
    e32, bound = X.bound_of(base.astype(np.float64), np.fft.irfft2(np.fft.rfft2(base, norm="ortho"), s=shape, norm="ortho"))
    d = np.abs(back.astype(np.float64) - base.astype(np.float64)[M.tile_index(n)])
    d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    print(f"70000 images round trip: err {d[k]:.3e} at image {k[0]}, bound {bound:.3e}")
    assert d[k] <= bound, (k, d[k], bound)


# ------------------------------------------------------------------ 2. the periodic blur
@pytest.mark.parametrize("name", F.CONV_IDS)
def test_periodic_convolution_and_adjoint_per_pixel(la, name):
    c = F.CONV_CASES[F.CONV_IDS.index(name)]
    op = la.PeriodicConvolve2D(c.shape, c.h, offset=c.offset)
    fwd, adj = F.conv_reference(name, False), F.conv_reference(name, True)
    got_f, got_a = op.matvec(fwd.x), op.rmatvec(adj.x)
    assert got_f.shape == fwd.x.shape and got_f.dtype == np.float32
    within(f"{name} H", got_f, fwd.ref64, fwd.bound, fwd.e32)
    within(f"{name} H^T", got_a, adj.ref64, adj.bound, adj.e32)
    flat = op @ fwd.x[0].ravel()
    assert flat.shape == (c.shape[0] * c.shape[1],)
    within(f"{name} H flat", flat.reshape(c.shape)[None], fwd.ref64[:1], fwd.bound, fwd.e32)
    within(f"{name} .H", (op.H @ adj.x[1].ravel()).reshape(c.shape)[None], adj.ref64[1:2], adj.bound, adj.e32)


@pytest.mark.parametrize("name", F.CONV_IDS)
def test_adjointness_from_the_device_outputs(la, name):
    """<H x, r> = <x, H^T r> summed in float64: each side is off by at most its bound per pixel times the 1-norm of the other operand."""
    c = F.CONV_CASES[F.CONV_IDS.index(name)]
    op = la.PeriodicConvolve2D(c.shape, c.h, offset=c.offset)
    fwd = F.conv_reference(name, False)
    x = fwd.x.astype(np.float64)
    r = np.random.default_rng(5).standard_normal(x.shape).astype(np.float32)
    hx = np.asarray(op.matvec(fwd.x), dtype=np.float64)
    htr = np.asarray(op.rmatvec(r), dtype=np.float64)
    _, bound_t = X.bound_of(F.periodic_direct(r.astype(np.float64), c.h, c.offset, True), F.periodic_direct(r, c.h, c.offset, True))
    lhs, rhs = float(np.sum(hx * r.astype(np.float64))), float(np.sum(x * htr))
    tol = fwd.bound * float(np.abs(r).sum()) + bound_t * float(np.abs(x).sum())
    print(f"adjointness {name}: <Hx, r> = {lhs:.9e}, <x, H^T r> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ------------------------------------------------------------------ 3. one MYULA step per pixel ("restart" mode)
def device_terms(la, c, m):
    if isinstance(c.op, tuple):
        pf = la.L2(Op=la.PeriodicConvolve2D(c.shape, m.h, offset=m.offset), b=m.y, sigma=m.sigma_f)
    else:
        pf = la.L2(Op=la.FourierSampling(c.shape, m.mask, transfer=m.transfer), b=m.y, sigma=m.sigma_f, weights=m.weights)
    if c.prior in ("tv", "aniso"):
        pg = la.TV(c.shape, sigma=m.weight, niter=c.K, isotropic=c.prior == "tv", bounds=c.box)
    elif c.prior == "l1":
        pg = la.L1(sigma=m.weight)
    elif c.prior == "wavelet":
        pg = la.WaveletL1(c.shape, sigma=m.weight, levels=F.WAVELET[2], wavelet=F.WAVELET[0])
    else:
        pg = None
    return pf, pg


PRIOR_KERNEL = {"mask-tv10-pipe": ("myula_step_pipe_kernel",), "mask-tv10-split": ("myula_step_split_kernel", "myula_step_tile_kernel")}


@pytest.mark.parametrize("name", [n for n in F.STEP_IDS if not n.startswith("grad")])
def test_myula_step_per_pixel(la, name):
    c = F.STEP_CASES[F.STEP_IDS.index(name)]
    m = F.step_problem(name)
    stages = F.step_reference(name)
    pf, pg = device_terms(la, c, m)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=F.N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        for it, st in enumerate(stages):
            smp.set_state(st.start)
            smp.step(1, noise=m.noise[it:it + 1])
            got = smp.get_state().cpu().numpy()
            within(f"{name} it {it} ({smp.kernel_name})", got, st.ref64, st.bound, st.e32)
        if name in PRIOR_KERNEL:
            assert smp.kernel_name in PRIOR_KERNEL[name], smp.kernel_name
    finally:
        smp.close()


@pytest.mark.parametrize("name", [n for n in F.STEP_IDS if n.startswith("grad")])
def test_gradient_alone_is_the_overwrite_form(la, name):
    c = F.STEP_CASES[F.STEP_IDS.index(name)]
    m = F.step_problem(name)
    st = F.step_reference(name)[0]
    pf, _ = device_terms(la, c, m)
    got = pf.grad(st.start)
    assert got.shape == st.start.shape
    within(name, got, st.ref64, st.bound, st.e32)


# ------------------------------------------------------------------ 4. the closed-form prox
@pytest.mark.parametrize("name", ["wmask-l1", "transfer-tvpos", "periodic15-aniso"])
def test_prox_per_pixel_and_optimality(la, name):
    c = F.STEP_CASES[F.STEP_IDS.index(name)]
    m = F.step_problem(name)
    pf, _ = device_terms(la, c, m)
    ref = F.SpectralRef(m.G, m.b, m.sigma_f)
    tau = 3.0 / ref.grad_lipschitz()
    want = ref.prox(m.x0, tau)
    A_, B_ = F.fold(m.G.astype(np.complex64), m.b.astype(np.complex64))
    r32 = np.fft.irfft2((np.fft.rfft2(m.x0, norm="ortho") + np.float32(tau * m.sigma_f) * F.half(B_).astype(np.complex64))
                        / (np.float32(1) + np.float32(tau * m.sigma_f) * F.half(A_).astype(np.float32)), s=c.shape, norm="ortho")
    assert r32.dtype == np.float32
    e32, bound = X.bound_of(want, r32)
    got = pf.prox(m.x0, tau)
    assert got.shape == m.x0.shape and got.dtype == np.float32
    within(f"prox {name}", got, want, bound, e32)
    p = got.astype(np.float64)
    res = float(np.max(np.abs(p - m.x0 + tau * ref.grad(p))))
    lim = bound * (1.0 + tau * ref.grad_lipschitz())
    print(f"prox {name}: optimality residual {res:.3e}, bound (1 + tau L) {lim:.3e}")
    assert res <= lim, (res, lim)


# ------------------------------------------------------------------ 5. Philox, sharding, SK-ROCK, SAPG
def problem(la, name="mask-tv10-split"):
    c = F.STEP_CASES[F.STEP_IDS.index(name)]
    m = F.step_problem(name)
    pf, pg = device_terms(la, c, m)
    return c, m, pf, pg


def test_philox_trajectory_matches_the_checker(la):
    c, m, pf, pg = problem(la)
    seed, nit, C_ = 3, 3, F.N_CHAINS
    ref, og = F.SpectralRef(m.G, m.b, m.sigma_f), F.prior_term(c, m, np.float64)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=C_, tau=m.tau, gamma=m.gamma, seed=seed)
    try:
        smp.set_state(m.x0)
        x = m.x0.astype(np.float64)
        for it in range(1, nit + 1):
            smp.step(1)
            x = P.myula_step(ref, og, x, m.tau, m.gamma, O.philox_normals(seed, it - 1, np.arange(C_), *c.shape).astype(np.float64))
            e = X.rel(smp.get_state().cpu().numpy(), x)
            print(f"Philox trajectory step {it}: rel {e:.3e} ({smp.kernel_name})")
            assert e <= STEP_TOL * it, (it, e)
    finally:
        smp.close()


def test_chain_sharding_reproduces_the_trajectories(la):
    """The noise of a chain depends on its global id only: four chains on one sampler are the chains of two samplers of two (chain_offset 0 and 2)."""
    c, m, pf, pg = problem(la)
    x0 = np.concatenate([m.x0, m.x0[:1] + 1.0])
    kw = dict(tau=m.tau, gamma=m.gamma, seed=9)
    whole = la.MYULASampler(pf, pg, c.shape, n_chains=4, **kw)
    whole.set_state(x0)
    whole.step(3)
    want = whole.get_state().cpu().numpy()
    whole.close()
    assert np.isfinite(want).all() and not np.array_equal(want, x0)
    for off in (0, 2):
        part = la.MYULASampler(pf, pg, c.shape, n_chains=2, chain_offset=off, **kw)
        part.set_state(x0[off:off + 2])
        part.step(3)
        np.testing.assert_array_equal(part.get_state().cpu().numpy(), want[off:off + 2])
        part.close()


def test_skrock_matches_the_restated_recursion(la):
    s, eta, nit = 3, 0.05, 2
    c, m, pf, pg = problem(la)
    ref, og = F.SpectralRef(m.G, m.b, m.sigma_f), F.prior_term(c, m, np.float64)
    Z = np.random.default_rng(4).standard_normal((nit,) + m.x0.shape)
    smp = la.SKROCKSampler(pf, pg, c.shape, n_stages=s, eta=eta, n_chains=F.N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        smp.set_state(m.x0)
        x = m.x0.astype(np.float64)
        for it in range(nit):
            x = P.skrock_iteration(ref, og, x, Z[it], m.tau, m.gamma, s, eta)
            smp.step(1, noise=Z[it:it + 1])
            e = X.rel(smp.get_state().cpu().numpy(), x)
            print(f"SK-ROCK iteration {it + 1}: rel {e:.3e} ({smp.kernel_name})")
            assert e <= STEP_TOL * (it + 1), (it, e)
    finally:
        smp.close()


def test_sapg_runs_and_moves_theta_inside_its_bounds(la):
    c, m, pf, pg = problem(la)
    n_updates, bounds = 3, (1e-3, 1e2)
    res = la.EstimatePriorWeight(pf, pg, m.x0, m.tau, m.gamma, n_updates, bounds, theta0=m.weight, step_scale=0.02, step_exponent=0.8, seed=5,
                                 n_chains=F.N_CHAINS, dims=c.shape)
    print(f"SAPG theta trace {res.theta_trace}")
    assert res.theta_trace.shape == (n_updates + 1,) and res.theta_trace[0] == m.weight
    assert np.all(np.isfinite(res.theta_trace))
    assert np.all((res.theta_trace[1:] > bounds[0]) & (res.theta_trace[1:] < bounds[1]))
    assert not np.allclose(res.theta_trace[1:], m.weight)


# ------------------------------------------------------------------ 6. energies
@pytest.mark.parametrize("name", ["mask-tv10-split", "transfer-tvpos", "periodic15-aniso"])
def test_energies_match_float64_and_repeat_bit_for_bit(la, name):
    from lmc_atomi_amd.proximal import _Problem
    c, m, pf, pg = problem(la, name)
    ref = F.SpectralRef(m.G, m.b, m.sigma_f)
    want = ref.value(m.x0)
    got = np.asarray(pf(m.x0))                                       # L2.__call__
    again = np.asarray(pf(m.x0))
    rel = np.max(np.abs(got - want) / np.abs(want))
    print(f"energies {name}: __call__ rel {rel:.2e}")
    assert got.shape == want.shape and rel < ENERGY_RTOL, (got, want)
    assert np.array_equal(got, again), "two evaluations of f differ: the reduction is not deterministic"
    assert abs(pf(m.x0[0]) - want[0]) < ENERGY_RTOL * abs(want[0])
    prob = _Problem(c.shape, pf.descriptor(), pg.prior_descriptor())
    f1, g1 = (t.cpu().numpy() for t in prob.energies(m.x0))          # lmc_energies
    f2, _ = (t.cpu().numpy() for t in prob.energies(m.x0))
    assert np.max(np.abs(f1 - want) / np.abs(want)) < ENERGY_RTOL and np.array_equal(f1, f2), (f1, f2, want)
    assert np.isfinite(g1).all() and (g1 > 0).all()
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, m.x0, tau=m.tau, gamma=m.gamma, niter=2, seed=3, n_chains=F.N_CHAINS, dims=c.shape)
    state = res.state.cpu().numpy()
    ef = res.energy_f.cpu().numpy()                                  # lmc_sampler_energies
    want_s = ref.value(state.reshape((F.N_CHAINS,) + c.shape))
    print(f"energies {name}: res.energy_f rel {np.max(np.abs(ef - want_s) / np.abs(want_s)):.2e}")
    assert np.max(np.abs(ef - want_s) / np.abs(want_s)) < ENERGY_RTOL, (ef, want_s)
    assert res.count > 0


# ------------------------------------------------------------------ 7. refusals
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
    cfg.tau, cfg.gamma, cfg.epsg = 1e-3, X.GAMMA, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return prob, cfg


def last_error():
    from lmc_atomi_amd import _dev
    return _dev.lib().lmc_last_error().decode()


REFUSED = [dict(ncvx_kind=1, ncvx_gamma=1.0), dict(tv_rtol=1e-4), dict(tv_warm=1, tv_niter=3)]


def test_c_abi_refusals(la):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    c, m, pf, _ = problem(la)
    shape = c.shape
    prior = la.TV(shape, sigma=0.3, niter=10).prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    stream = _dev.stream_ptr(x.device)
    for fields in REFUSED:
        prob, cfg = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert prob.c.data_kind == _capi.DATA_SPECTRAL
        for create in (lambda h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h))):
            hnd = C.c_void_p()
            rc = create(hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == LMC_E_UNSUPPORTED and msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, stream)
        assert rc == LMC_E_UNSUPPORTED and last_error(), (fields, rc, last_error())
    # the samplers without a form of the term
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "spectral" in last_error() and not hnd.value, (rc, last_error())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "spectral" in last_error() and not hnd.value, (rc, last_error())
    # fields the kind does not read must be empty; a size the transforms do not take
    keep = np.ones(4, dtype=np.float32)
    for fields in (dict(mask_dev=x.data_ptr()), dict(h_host=_dev.fptr(keep)), dict(kh=3), dict(kw=3), dict(oy=1), dict(ox=1), dict(psf_kh=3), dict(psf_kw=3),
                   dict(psf_oy=1), dict(psf_ox=1), dict(y_dev=None)):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_INVALID and last_error() and not hnd.value, (fields, rc, last_error())
    for fields in (dict(H=48), dict(W=4), dict(H=2048, W=8)):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_UNSUPPORTED and "powers of two" in last_error() and not hnd.value, (fields, rc, last_error())
    # the stateless transforms
    half = torch.zeros((2, shape[0], shape[1] // 2 + 1, 2), dtype=torch.float32, device="cuda")
    assert lib.lmc_rfft2(_dev.ptr(x), _dev.ptr(half), 2, shape[0], shape[1], stream) == 0, last_error()
    assert lib.lmc_rfft2(_dev.ptr(x), _dev.ptr(x), 2, shape[0], shape[1], stream) == LMC_E_INVALID
    assert lib.lmc_rfft2(_dev.ptr(x), _dev.ptr(half), 0, shape[0], shape[1], stream) == LMC_E_INVALID
    assert lib.lmc_rfft2(_dev.ptr(x), _dev.ptr(half), 2, 48, 64, stream) == LMC_E_UNSUPPORTED and last_error()
    assert lib.lmc_irfft2(_dev.ptr(half), _dev.ptr(out), 2, 64, 4, stream) == LMC_E_UNSUPPORTED and last_error()
    assert lib.lmc_spectral_filter(_dev.ptr(x), _dev.ptr(out), 2, shape[0], shape[1], None, stream) == LMC_E_INVALID and last_error()
    assert lib.lmc_spectral_filter(_dev.ptr(x), _dev.ptr(out), 2, 2048, 8, _dev.ptr(half), stream) == LMC_E_UNSUPPORTED
    # what is not refused: the problem as it stands (iterations_per_launch is ignored), a forced variant of the prior launch, the closed-form prox
    for fields in (dict(), dict(iterations_per_launch=2), dict(step_variant=1)):
        prob_ok, cfg_ok = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert lib.lmc_myula_create(C.byref(cfg_ok), C.byref(hnd)) == 0, last_error()
        assert lib.lmc_sampler_step(hnd, 1, None, stream) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
    assert lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 0, 0, None, stream) == 0, last_error()
    torch.cuda.synchronize()


def test_python_refusals(la):
    c, m, pf, pg = problem(la)
    shape = c.shape
    kw = dict(n_chains=2, tau=1e-3, gamma=X.GAMMA)
    with pytest.raises(NotImplementedError):
        la.MYMALASampler(pf, pg, shape, **kw)
    with pytest.raises(NotImplementedError):
        la.UnadjustedLangevinPrimalDual(pf, la.L21(ndim=2, sigma=0.3), la.Gradient(shape), m.x0[0].ravel(), tau=0.1, mu=0.1, niter=2)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=1e-4), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=3, warm=True), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=3), shape, tv_warm=True, **kw)
    with pytest.raises(NotImplementedError):
        la.SKROCKSampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=1e-4), shape, n_stages=3, **kw)
    with pytest.raises(NotImplementedError):
        la.Poisson(pf.Op, np.ones(shape), 1.0)
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(dims=shape, Op=pf.Op, b=m.y, sigma=1.0)
    la.MYULASampler(pf, pg, shape, **kw).close()
    la.SKROCKSampler(pf, pg, shape, n_stages=3, **kw).close()
