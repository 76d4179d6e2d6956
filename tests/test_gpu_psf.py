"""GPU parity of the large point-spread functions (`la.PSF`, LMC_DATA_PSF / POISSON_PSF / WL2_PSF in include/lmc_atomi.h) against the references of
tests/_psf_ref.py: the operator and its adjoint per pixel in both forms, adjointness, more than 65535 images, one MYULA step per pixel for the three
data terms and the priors that take another kernel in the prior launch, the Philox path, chain sharding, SK-ROCK, SAPG, the energies, and the refusals
of the C ABI and of the Python surface.

Per pixel: max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|)) over every chain and pixel, e32 measured on the checker's float32 replay
(tests/_pixel.py).  Trajectories: the project's rel-L2 1e-5 x (step index); energies: rtol 5e-5."""
import ctypes as C

import numpy as np
import pytest

import _many as M
import _pixel as X
import _poisson_ref as P
import _psf_ref as R
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
    err, where = R.worst(got, ref64)
    print(f"pixel {what}: err {err:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert err <= bound, (what, err, bound, where)
    return err


# ------------------------------------------------------------------ 1. the operator, both directions, both forms
FORMS = [(c.name, None) for c in R.CASES] + [(c.name, False) for c in R.SEP_CASES]


@pytest.mark.parametrize("name,separable", FORMS, ids=[f"{n}-{'auto' if s is None else 'general'}" for n, s in FORMS])
def test_operator_and_adjoint_per_pixel(la, name, separable):
    c = R.CASES[R.IDS.index(name)]
    op = la.PSF(c.shape, c.h, offset=c.offset, separable=separable)
    assert (op.factors is not None) == (c.separable and separable is None)
    fwd, adj = R.op_reference(name, False), R.op_reference(name, True)
    got_f = op.matvec(fwd.x)
    got_a = op.rmatvec(adj.x)
    assert got_f.shape == fwd.x.shape and got_f.dtype == np.float32
    within(f"{name} H", got_f, fwd.ref64, fwd.bound, fwd.e32)
    within(f"{name} H^T", got_a, adj.ref64, adj.bound, adj.e32)
    # the pylops protocol: flat vectors, .H, @
    flat = op @ fwd.x[0].ravel()
    assert flat.shape == (c.shape[0] * c.shape[1],)
    within(f"{name} H flat", flat.reshape(c.shape)[None], fwd.ref64[:1], fwd.bound, fwd.e32)
    within(f"{name} .H", (op.H @ adj.x[1].ravel()).reshape(c.shape)[None], adj.ref64[1:2], adj.bound, adj.e32)


@pytest.mark.parametrize("name", R.IDS)
def test_adjointness_from_the_device_outputs(la, name):
    """<H x, r> = <x, H^T r> summed in float64: each side is off by at most its bound per pixel times the 1-norm of the other operand."""
    c = R.CASES[R.IDS.index(name)]
    op = la.PSF(c.shape, c.h, offset=c.offset)
    fwd, adj = R.op_reference(name, False), R.op_reference(name, True)
    x = fwd.x.astype(np.float64)
    r = np.random.default_rng(5).standard_normal(x.shape).astype(np.float32)
    hx = np.asarray(op.matvec(fwd.x), dtype=np.float64)
    htr = np.asarray(op.rmatvec(r), dtype=np.float64)
    r_ref = R.O.blur_adjoint(r.astype(np.float64), c.h.astype(np.float64), c.offset)
    _, bound_t = X.bound_of(r_ref, R.O.blur_adjoint(r, c.h, c.offset))
    lhs, rhs = float(np.sum(hx * r.astype(np.float64))), float(np.sum(x * htr))
    tol = fwd.bound * float(np.abs(r).sum()) + bound_t * float(np.abs(x).sum())
    print(f"adjointness {name}: <Hx, r> = {lhs:.9e}, <x, H^T r> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


def test_more_images_than_a_grid_dimension_holds(la):
    """70000 images of 4 x 4 under an 11 x 9 PSF: image c is pattern c % 7, so an image index that wraps or loses its chunk shows as another pattern."""
    n, shape = 70000, (4, 4)
    h = X.f32(R.random_taps(11, 9, 9))
    off = (3, 6)
    base = X.f32(M.patterns(shape, seed=4))
    op = la.PSF(shape, h, offset=off)
    x = M.tile_dev(base, n)
    for adjoint, fn, oracle in ((False, op.matvec, O.blur), (True, op.rmatvec, O.blur_adjoint)):
        r64 = oracle(base.astype(np.float64), h.astype(np.float64), off)
        e32, bound = X.bound_of(r64, oracle(base, h, off))
        got = fn(x).cpu().numpy()
        assert got.shape == (n,) + shape
        d = np.abs(got.astype(np.float64) - r64[M.tile_index(n)])
        d = np.where(np.isfinite(d), d, np.inf)
        k = np.unravel_index(int(np.argmax(d)), d.shape)
        print(f"70000 images adjoint={adjoint}: err {d[k]:.3e} at image {k[0]} (pattern {k[0] % M.P}), bound {bound:.3e}")
        assert d[k] <= bound, (k, d[k], bound)


# ------------------------------------------------------------------ 2. one MYULA step per pixel ("restart" mode)
def device_terms(la, c, m, separable=None):
    op = la.PSF(c.shape, m.h, offset=m.offset, separable=separable)
    if c.term == "pois":
        pf = la.Poisson(op, m.y, m.aux, sigma=m.sigma_f)
    elif c.term == "wl2":
        pf = la.L2(Op=op, b=m.y, sigma=m.sigma_f, weights=m.aux)
    else:
        pf = la.L2(Op=op, b=m.y, sigma=m.sigma_f)
    if c.prior in ("tv", "aniso"):
        pg = la.TV(c.shape, sigma=m.weight, niter=c.K, isotropic=c.prior == "tv", bounds=c.box)
    elif c.prior == "l1":
        pg = la.L1(sigma=m.weight)
    else:
        pg = None
    return pf, pg


PRIOR_KERNEL = {"l2-tv10-pipe": ("myula_step_pipe_kernel",), "l2-tv10-split": ("myula_step_split_kernel", "myula_step_tile_kernel")}


@pytest.mark.parametrize("name", [n for n in R.STEP_IDS if n != "l2-grad"])
def test_myula_step_per_pixel(la, name):
    c = R.STEP_CASES[R.STEP_IDS.index(name)]
    m = R.step_problem(name)
    stages = R.step_reference(name)
    pf, pg = device_terms(la, c, m)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=R.N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
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


def test_gradient_alone_is_the_overwrite_form(la):
    name = "l2-grad"
    c = R.STEP_CASES[R.STEP_IDS.index(name)]
    m = R.step_problem(name)
    st = R.step_reference(name)[0]
    for separable in (None, False):
        pf, _ = device_terms(la, c, m, separable)
        got = pf.grad(st.start)
        assert got.shape == st.start.shape
        within(f"{name} separable={separable}", got, st.ref64, st.bound, st.e32)


# ------------------------------------------------------------------ 3. Philox, sharding
def gaussian_problem(la, name="l2-tv10-pipe"):
    c = R.STEP_CASES[R.STEP_IDS.index(name)]
    m = R.step_problem(name)
    pf, pg = device_terms(la, c, m)
    return c, m, pf, pg


def test_philox_trajectory_matches_the_checker(la):
    c, m, pf, pg = gaussian_problem(la)
    seed, nit, C_ = 3, 3, R.N_CHAINS
    prior = {"kind": "tv", "sigma": m.weight, "niter": c.K, "t": m.gamma}
    noise = lambda k: O.philox_normals(seed, k, np.arange(C_), *c.shape).astype(np.float64)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=C_, tau=m.tau, gamma=m.gamma, seed=seed)
    try:
        smp.set_state(m.x0)
        for it in range(1, nit + 1):
            smp.step(1)
            ref = O.myula_batched(m.x0.astype(np.float64), m.y.astype(np.float64), m.h.astype(np.float64), m.offset, m.sigma_f, m.tau, m.gamma, prior, it, noise)
            e = X.rel(smp.get_state().cpu().numpy(), ref)
            print(f"Philox trajectory step {it}: rel {e:.3e} ({smp.kernel_name})")
            assert e <= STEP_TOL * it, (it, e)
    finally:
        smp.close()


def test_chain_sharding_reproduces_the_trajectories(la):
    """The noise of a chain depends on its global id only: four chains on one sampler are the chains of two samplers of two (chain_offset 0 and 2)."""
    c, m, pf, pg = gaussian_problem(la)
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


# ------------------------------------------------------------------ 4. SK-ROCK, SAPG
def test_skrock_matches_the_restated_recursion(la):
    s, eta, nit = 3, 0.05, 2
    c, m, pf, pg = gaussian_problem(la, "l2-tv10-split")
    ref, og = R.data_term(c, m, np.float64), R.prior_term(c, m, np.float64)
    Z = np.random.default_rng(4).standard_normal((nit,) + m.x0.shape)
    smp = la.SKROCKSampler(pf, pg, c.shape, n_stages=s, eta=eta, n_chains=R.N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
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
    c, m, pf, pg = gaussian_problem(la, "l2-tv10-split")
    n_updates, bounds = 3, (1e-3, 1e2)
    res = la.EstimatePriorWeight(pf, pg, m.x0, m.tau, m.gamma, n_updates, bounds, theta0=m.weight, step_scale=0.02, step_exponent=0.8, seed=5,
                                 n_chains=R.N_CHAINS, dims=c.shape)
    print(f"SAPG theta trace {res.theta_trace}")
    assert res.theta_trace.shape == (n_updates + 1,) and res.theta_trace[0] == m.weight
    assert np.all(np.isfinite(res.theta_trace))
    assert np.all((res.theta_trace[1:] > bounds[0]) & (res.theta_trace[1:] < bounds[1]))
    assert not np.allclose(res.theta_trace[1:], m.weight)


# ------------------------------------------------------------------ 5. energies
def f_reference(c, m, x):
    x = np.asarray(x, dtype=np.float64)
    if c.term == "l2":
        r = O.blur(x, m.h.astype(np.float64), m.offset) - m.y.astype(np.float64)
        return 0.5 * m.sigma_f * (r * r).sum(axis=(-2, -1))
    return np.asarray(R.data_term(c, m, np.float64)(x))


@pytest.mark.parametrize("name", ["l2-tv10-split", "wl2-tvbox", "pois-tvpos-gauss21", "l2-l1-33"])
def test_energies_match_float64_and_repeat_bit_for_bit(la, name):
    from lmc_atomi_amd.proximal import _Problem
    c, m, pf, pg = gaussian_problem(la, name)
    want = f_reference(c, m, m.x0)
    got = np.asarray(pf(m.x0))                                       # L2.__call__ / Poisson.__call__
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
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, m.x0, tau=m.tau, gamma=m.gamma, niter=2, seed=3, n_chains=R.N_CHAINS, dims=c.shape)
    state = res.state.cpu().numpy()
    ef = res.energy_f.cpu().numpy()                                  # lmc_sampler_energies
    want_s = f_reference(c, m, state.reshape((R.N_CHAINS,) + c.shape))
    print(f"energies {name}: res.energy_f rel {np.max(np.abs(ef - want_s) / np.abs(want_s)):.2e}")
    assert np.max(np.abs(ef - want_s) / np.abs(want_s)) < ENERGY_RTOL, (ef, want_s)
    assert res.count > 0


# ------------------------------------------------------------------ 6. refusals
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


@pytest.mark.parametrize("name", ["l2-tv10-split", "wl2-tvbox", "pois-tvpos-gauss21"])
def test_c_abi_refusals(la, name):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    c, m, pf, _ = gaussian_problem(la, name)
    shape = c.shape
    prior = la.TV(shape, sigma=0.3, niter=10).prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    stream = _dev.stream_ptr(x.device)
    for fields in REFUSED:
        prob, cfg = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert prob.c.data_kind in _capi.PSF_KINDS
        for create in (lambda h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h))):
            hnd = C.c_void_p()
            rc = create(hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == LMC_E_UNSUPPORTED and msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, stream)
        assert rc == LMC_E_UNSUPPORTED and last_error(), (fields, rc, last_error())
    # the samplers and the entry point without a PSF form
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "large PSF" in last_error() and not hnd.value, (rc, last_error())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and last_error() and not hnd.value, (rc, last_error())
    ws = torch.empty(lib.lmc_l2_prox_workspace_bytes(2, *shape), dtype=torch.uint8, device="cuda")
    rc = lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 5, 0, _dev.ptr(ws), stream)
    assert rc == LMC_E_UNSUPPORTED and last_error(), (rc, last_error())
    # bad geometry, no taps, and the geometry of the small blur beside the PSF's
    kh, kw = m.h.shape
    for fields in (dict(psf_kh=34), dict(psf_kw=0), dict(psf_oy=kh), dict(psf_ox=kw), dict(psf_separable=3), dict(psf_separable=-1), dict(h_host=None),
                   dict(kh=5, kw=5), dict(kh=kh, kw=kw), dict(oy=1), dict(ox=1)):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_INVALID and last_error() and not hnd.value, (fields, rc, last_error())
    if lib.lmc_psf_separable(_dev.fptr(m.h), kh, kw, None, None) == 0:
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, psf_separable=1)
        assert lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd)) == LMC_E_INVALID and not hnd.value
    # what is not refused: the problem as it stands (iterations_per_launch is ignored), every forced variant the prior launch has
    for fields in (dict(), dict(iterations_per_launch=2), dict(step_variant=1)):
        prob_ok, cfg_ok = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert lib.lmc_myula_create(C.byref(cfg_ok), C.byref(hnd)) == 0, last_error()
        assert lib.lmc_sampler_step(hnd, 1, None, stream) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
    torch.cuda.synchronize()


def test_psf_apply_refuses_bad_arguments(la):
    import torch
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    x = torch.zeros((2, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    h = X.f32(R.random_taps(5, 7, 1))
    st = _dev.stream_ptr(x.device)
    call = lambda xp, op_, kh, kw, oy, ox, sep: lib.lmc_psf_apply(xp, op_, 2, 8, 8, _dev.fptr(h), kh, kw, oy, ox, 0, sep, st)
    assert call(_dev.ptr(x), _dev.ptr(out), 5, 7, 2, 3, 0) == 0, last_error()
    assert call(_dev.ptr(x), _dev.ptr(x), 5, 7, 2, 3, 0) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), 34, 1, 0, 0, 0) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), 5, 7, 5, 0, 0) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), 5, 7, 0, 7, 0) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), 5, 7, 2, 3, 1) == LMC_E_INVALID and "outer product" in last_error()
    assert call(_dev.ptr(x), _dev.ptr(out), 5, 7, 2, 3, 4) == LMC_E_INVALID
    torch.cuda.synchronize()


def test_python_refusals(la):
    c, m, pf, pg = gaussian_problem(la, "l2-tv10-split")
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
        pf.prox(m.x0[0], 1.0)
    with pytest.raises(NotImplementedError):
        la.L2_ncvx_tv(dims=shape, Op=pf.Op, b=m.y, sigma=1.0)
    with pytest.raises(ValueError):
        la.Convolve2D(shape, np.ones((11, 11)) / 121.0)
    la.MYULASampler(pf, pg, shape, **kw).close()
    la.SKROCKSampler(pf, pg, shape, n_stages=3, **kw).close()
