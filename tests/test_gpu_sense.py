"""GPU parity of the multi-coil SENSE data term (`la.MultiCoilFourierSampling`; LMC_DATA_SENSE in include/lmc_atomi.h) against the references of
tests/_sense_ref.py: the operator and its adjoint per bin and pixel, the gradient alone (the overwrite form) and under a prior (the three-step form),
one MYULA step per pixel for the priors that take another kernel in the prior launch, SK-ROCK, SAPG, the energies, 32 coils, more than 65535 images,
determinism, chain sharding, the Philox trajectory, and the refusals of the C ABI and of the Python surface.

Per pixel / bin: max |got - ref64| <= max(3 e32, 2 ulp32(max |ref64|)) over every chain and pixel, e32 measured on numpy's single-precision replay
(tests/_pixel.py's bound).  Trajectory: the project's rel-L2 1e-5 x (step index), beside the per-pixel figure; energies: rtol 5e-5 (the tolerance of
tests/test_gpu_fourier.py)."""
import ctypes as C

import numpy as np
import pytest

import _many as M
import _pixel as X
import _poisson_ref as P
import _sense_ref as S
import _skrock_pixel as K
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
    err, where = S.worst(got, ref64)
    print(f"pixel {what}: err {err:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert err <= bound, (what, err, bound, where)
    return err


def terms_of(la, m, shape):
    op = la.MultiCoilFourierSampling(shape, m.S, m.M)
    return op, la.L2(Op=op, b=m.b, sigma=m.sigma_f)


# ------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("wkind", S.WEIGHTS)
@pytest.mark.parametrize("name", S.IDS)
def test_operator_and_adjoint_per_bin_and_pixel(la, name, wkind):
    c = S.case(name)
    fw, ad = S.forward_reference(c.shape, c.n_coils, wkind), S.adjoint_reference(c.shape, c.n_coils, wkind)
    op = la.MultiCoilFourierSampling(c.shape, S.maps(c.shape, c.n_coils), S.weight(c.shape, wkind))
    got = op.matvec(fw.x)
    n = c.n_coils * c.shape[0] * c.shape[1]
    assert got.shape == (3, n) and got.dtype == np.complex64
    within(f"A {name} {wkind}", S.ri(got.reshape((3, c.n_coils) + c.shape)), fw.ref64, fw.bound, fw.e32)
    back = op.rmatvec(ad.x)
    assert back.shape == (3, c.shape[0] * c.shape[1]) and back.dtype == np.float32
    within(f"A^H {name} {wkind}", back.reshape((3,) + c.shape), ad.ref64, ad.bound, ad.e32)
    if wkind == "weighted":      # the flat forms of one image: @ and .H
        one = op @ fw.x[1].ravel()
        within(f"A {name} flat", S.ri(one.reshape((1, c.n_coils) + c.shape)), fw.ref64[1:2], fw.bound, fw.e32)
        within(f"A.H {name} flat", (op.H @ ad.x[2].ravel()).reshape((1,) + c.shape), ad.ref64[2:3], ad.bound, ad.e32)


# ------------------------------------------------------------------ 2. the gradient: alone (the last launch writes a x - t sigma_f g) and under a prior
@pytest.mark.parametrize("wkind", S.WEIGHTS)
@pytest.mark.parametrize("name", S.IDS)
def test_gradient_alone_is_the_overwrite_form(la, name, wkind):
    from lmc_atomi_amd.proximal import _Problem
    c = S.case(name)
    m = S.problem(c.shape, c.n_coils, wkind)
    ref = S.grad_reference(c.shape, c.n_coils, wkind)
    _, pf = terms_of(la, m, c.shape)
    got = pf.grad(m.x0)
    assert got.shape == m.x0.shape and got.dtype == np.float32
    within(f"grad {name} {wkind}", got, ref.ref64, ref.bound, ref.e32)
    # lmc_fused_eval with a = 1, b = s = 0: x - t grad f(x)
    t = m.tau
    r64 = m.x0.astype(np.float64) - t * ref.ref64
    r32 = m.x0 - np.float32(t) * ref.ref32
    assert r32.dtype == np.float32
    e32, bound = X.bound_of(r64, r32)
    got = _Problem(c.shape, pf.descriptor()).eval(m.x0, 1.0, t, 0.0, 0.0)
    within(f"x - t grad {name} {wkind}", got, r64, bound, e32)


@pytest.mark.parametrize("name", S.IDS)
def test_gradient_under_a_prior_is_the_three_step_form(la, name):
    """lmc_fused_eval with b != 0: the gradient image, the step of the problem without a data term (the l1 prox), out -= t sigma_f g."""
    from lmc_atomi_amd.proximal import _Problem
    c = S.case(name)
    m = S.problem(c.shape, c.n_coils, "weighted")
    _, pf = terms_of(la, m, c.shape)
    a, t, b, pt = 0.8, m.tau, 0.2, m.gamma
    res = []
    for dtype in (np.float64, np.float32):
        T = np.dtype(dtype).type
        x = m.x0.astype(dtype)
        thr = T(X.L1_WEIGHT * pt)
        prox = np.sign(x) * np.maximum(np.abs(x) - thr, T(0))
        r = T(a) * x - T(t) * S.term(m, dtype).grad(x) + T(b) * prox
        assert r.dtype == np.dtype(dtype)
        res.append(r)
    e32, bound = X.bound_of(res[0], res[1])
    got = _Problem(c.shape, pf.descriptor(), la.L1(sigma=X.L1_WEIGHT).prior_descriptor()).eval(m.x0, a, t, b, pt)
    within(f"a x - t grad + b prox {name}", got, res[0], bound, e32)


# ------------------------------------------------------------------ 3. one MYULA step per pixel ("restart" mode)
def device_prior(la, c):
    w = S.prior_weight(c)
    if c.prior in ("tv", "aniso"):
        return la.TV(c.shape, sigma=w, niter=c.K, isotropic=c.prior == "tv", bounds=c.box)
    if c.prior == "l1":
        return la.L1(sigma=w)
    if c.prior == "wavelet":
        return la.WaveletL1(c.shape, sigma=w, levels=S.WAVELET[2], wavelet=S.WAVELET[0])
    if c.prior == "tgv":
        return la.TGV(c.shape, sigma=w, alpha0=S.TGV_ALPHA0, niter=S.TGV_K)
    return None


@pytest.mark.parametrize("name", S.STEP_IDS)
def test_myula_step_per_pixel(la, name):
    c = S.step_case(name)
    m = S.problem(c.shape, c.n_coils, c.wkind)
    stages = S.step_reference(name)
    _, pf = terms_of(la, m, c.shape)
    smp = la.MYULASampler(pf, device_prior(la, c), c.shape, n_chains=S.N_CHAINS, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        for it, st in enumerate(stages):
            smp.set_state(st.start)
            smp.step(1, noise=m.noise[it:it + 1])
            got = smp.get_state().cpu().numpy()
            within(f"step {name} it {it} ({smp.kernel_name})", got, st.ref64, st.bound, st.e32)
        if name == "tv10-pipe":
            assert "pipe" in smp.kernel_name, smp.kernel_name
    finally:
        smp.close()


# ------------------------------------------------------------------ 4. SK-ROCK, SAPG
class _Terms:
    """What tests/_skrock_pixel.py's replays read: grad f, prox_{gamma g}, the fused launch over them and the drift, in `dtype`."""

    def __init__(self, m, c, dtype):
        self.dtype, self.gamma = np.dtype(dtype), m.gamma
        self.pf, self.pg = S.term(m, dtype), S.prior_term(c, dtype)

    def grad(self, x):
        return self.pf.grad(x)

    def prox(self, x):
        return self.pg.prox(x, self.gamma)

    def launch(self, a, t, b, s, x, n):
        T = self.dtype.type
        return T(a) * x - T(t) * self.grad(x) + T(b) * self.prox(x) + T(s) * n

    def drift(self, x):
        return -self.grad(x) - (x - self.prox(x)) / self.dtype.type(self.gamma)

    def advance(self, v, t):
        return P.myula_step(self.pf, self.pg, v, t, self.gamma, np.zeros_like(v), dtype=self.dtype)


def test_skrock_iteration_per_pixel(la):
    """One iteration of three stages: float64 definition; float32 in the definition's form and in the launches' form (tests/_skrock_pixel.py)."""
    s, eta = 3, K.ETA
    c = S.step_case("tv10-box")._replace(name="skrock", box=None)
    m = S.problem(c.shape, c.n_coils, c.wkind)
    _, pf = terms_of(la, m, c.shape)
    Z = m.noise[0]
    delta = float(np.float32(K.STEP_FRACTION * K.step_factor(s) / (S.term(m).grad_lipschitz() + 1.0 / m.gamma)))
    t64, t32 = _Terms(m, c, np.float64), _Terms(m, c, np.float32)
    r64 = K.iteration_definition(t64.advance, m.x0, Z, delta, s, np.float64)
    ra = K.iteration_definition(t32.advance, m.x0, Z, delta, s, np.float32)
    rb = K.iteration_launch(t32, m.x0, Z, delta, s)
    st = K.make_stage(m.x0, r64, ra, rb, 0.0, True)
    smp = la.SKROCKSampler(pf, device_prior(la, c), c.shape, n_stages=s, eta=eta, n_chains=S.N_CHAINS, tau=delta, gamma=m.gamma, noise="injected")
    try:
        smp.set_state(m.x0)
        smp.step(1, noise=Z[None])
        got = smp.get_state().cpu().numpy()
        print(f"SK-ROCK rel {X.rel(got, r64):.3e} ({smp.kernel_name})")
        within("SK-ROCK 3 stages", got, st.ref64, st.bound, st.e32)
    finally:
        smp.close()


def test_sapg_follows_the_float64_replay(la):
    """Two updates: the chains by the float64 MYULA step of the reference (Philox field of the checker, the prior at the current theta), the statistic the
    mean TV value of the chains in float64, theta by the host update `la.sapg_update`; the project's relative tolerance 1e-5 x (update index)."""
    c = S.step_case("tv10-box")._replace(box=None)
    m = S.problem(c.shape, c.n_coils, c.wkind)
    _, pf = terms_of(la, m, c.shape)
    pg = device_prior(la, c)
    n_updates, bounds, seed = 2, (1e-3, 1e2), 5
    kw = dict(theta_bounds=bounds, step_scale=0.02, step_exponent=0.8)
    res = la.EstimatePriorWeight(pf, pg, m.x0, m.tau, m.gamma, n_updates, bounds, theta0=X.TAU_REG, step_scale=0.02, step_exponent=0.8, seed=seed,
                                 n_chains=S.N_CHAINS, dims=c.shape)
    dim, k = la.sapg_dimension(pg, c.shape)
    ref = S.term(m)
    theta, x, trace = X.TAU_REG, m.x0.astype(np.float64), [X.TAU_REG]
    for n in range(n_updates):
        xi = O.philox_normals(seed, n, np.arange(S.N_CHAINS), *c.shape).astype(np.float64)
        x = P.myula_step(ref, P.TVRef(c.shape, theta, c.K), x, m.tau, m.gamma, xi)
        gbar = float(np.mean(P.TVRef(c.shape, 1.0, c.K).value(x)))
        theta = la.sapg_update(theta, gbar, n, dim, k, **kw)
        trace.append(theta)
    trace = np.array(trace)
    print(f"SAPG theta trace {res.theta_trace} (float64 replay {trace})")
    assert res.theta_trace.shape == (n_updates + 1,) and res.theta_trace[0] == X.TAU_REG
    assert np.all((trace[1:] > bounds[0]) & (trace[1:] < bounds[1])) and not np.allclose(trace[1:], X.TAU_REG), "the updates move theta and none is clamped"
    err = np.abs(res.theta_trace - trace) / trace
    assert np.all(err[1:] < STEP_TOL * np.arange(1, n_updates + 1)), err


# ------------------------------------------------------------------ 5. energies
@pytest.mark.parametrize("name", ["8x8x1", "16x8x3", "8x1024x2", "128x256x4"])
def test_energies_match_float64_and_repeat_bit_for_bit(la, name):
    from lmc_atomi_amd.proximal import _Problem
    c = S.case(name)
    m = S.problem(c.shape, c.n_coils, "weighted")
    _, pf = terms_of(la, m, c.shape)
    pg = la.TV(c.shape, sigma=X.TAU_REG, niter=10)
    want = S.term(m).value(m.x0)
    got, again = np.asarray(pf(m.x0)), np.asarray(pf(m.x0))                  # L2.__call__
    rel = np.max(np.abs(got - want) / np.abs(want))
    print(f"energies {name}: __call__ rel {rel:.2e}")
    assert got.shape == want.shape and rel < ENERGY_RTOL, (got, want)
    assert np.array_equal(got, again), "two evaluations of f differ: the reduction is not deterministic"
    prob = _Problem(c.shape, pf.descriptor(), pg.prior_descriptor())
    f1, g1 = (t.cpu().numpy() for t in prob.energies(m.x0))                 # lmc_energies
    assert np.max(np.abs(f1 - want) / np.abs(want)) < ENERGY_RTOL, (f1, want)
    assert np.isfinite(g1).all() and (g1 > 0).all()
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, m.x0, tau=m.tau, gamma=m.gamma, niter=2, seed=3, n_chains=S.N_CHAINS, dims=c.shape)
    state = res.state.cpu().numpy()
    ef = res.energy_f.cpu().numpy()                                          # lmc_sampler_energies
    want_s = S.term(m).value(state.reshape((S.N_CHAINS,) + c.shape))
    print(f"energies {name}: res.energy_f rel {np.max(np.abs(ef - want_s) / np.abs(want_s)):.2e}")
    assert np.max(np.abs(ef - want_s) / np.abs(want_s)) < ENERGY_RTOL, (ef, want_s)


# ------------------------------------------------------------------ 6. coil counts, many images
def test_thirty_two_coils(la):
    shape, nc = (16, 16), 32
    m = S.problem(shape, nc, "weighted")
    ref = S.grad_reference(shape, nc, "weighted")
    _, pf = terms_of(la, m, shape)
    within("grad 16x16x32", pf.grad(m.x0), ref.ref64, ref.bound, ref.e32)
    want = S.term(m).value(m.x0)
    got = np.asarray(pf(m.x0))
    assert np.max(np.abs(got - want) / np.abs(want)) < ENERGY_RTOL, (got, want)


def test_more_images_than_a_grid_dimension_holds(la):
    """70000 images of 8 x 8 with one coil: image c is pattern c % 7, so an image index that wraps or loses its chunk shows as another pattern."""
    n, shape = 70000, (8, 8)
    m = S.problem(shape, 1, "weighted")
    base = M.patterns(shape, seed=4)
    base = X.f32(base - base.mean(axis=(-2, -1), keepdims=True))
    r64, r32 = S.term(m).grad(base), S.term(m, np.float32).grad(base)
    e32, bound = X.bound_of(r64, r32)
    _, pf = terms_of(la, m, shape)
    got = pf.grad(M.tile_dev(base, n)).cpu().numpy()
    assert got.shape == (n, 8, 8)
    d = np.abs(got.astype(np.float64) - r64[M.tile_index(n)])
    d = np.where(np.isfinite(d), d, np.inf)
    k = np.unravel_index(int(np.argmax(d)), d.shape)
    print(f"70000 images grad: err {d[k]:.3e} at image {k[0]} (pattern {k[0] % M.P}), e32 {e32:.3e}, bound {bound:.3e}")
    assert d[k] <= bound, (k, d[k], bound)


# ------------------------------------------------------------------ 7. determinism, sharding, the Philox trajectory
def problem(la, name="tv10-box"):
    c = S.step_case(name)._replace(box=None)
    m = S.problem(c.shape, c.n_coils, c.wkind)
    _, pf = terms_of(la, m, c.shape)
    return c, m, pf, device_prior(la, c)


def test_two_runs_give_equal_bits(la):
    c, m, pf, pg = problem(la)
    outs = []
    for _ in range(2):
        smp = la.MYULASampler(pf, pg, c.shape, n_chains=S.N_CHAINS, tau=m.tau, gamma=m.gamma, seed=11)
        smp.set_state(m.x0)
        smp.step(3)
        outs.append((smp.get_state().cpu().numpy(), np.asarray(pf.grad(m.x0)), np.asarray(pf(m.x0))))
        smp.close()
    for a, b in zip(*outs):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)


def test_chain_sharding_reproduces_the_trajectories(la):
    """The noise of a chain depends on its global id only: three chains on one sampler are the chains of a sampler of two and one of one."""
    c, m, pf, pg = problem(la)
    kw = dict(tau=m.tau, gamma=m.gamma, seed=9)
    whole = la.MYULASampler(pf, pg, c.shape, n_chains=3, **kw)
    whole.set_state(m.x0)
    whole.step(3)
    want = whole.get_state().cpu().numpy()
    whole.close()
    assert np.isfinite(want).all() and not np.array_equal(want, m.x0)
    for off, n in ((0, 2), (2, 1)):
        part = la.MYULASampler(pf, pg, c.shape, n_chains=n, chain_offset=off, **kw)
        part.set_state(m.x0[off:off + n])
        part.step(3)
        np.testing.assert_array_equal(part.get_state().cpu().numpy(), want[off:off + n])
        part.close()


def test_philox_trajectory_matches_the_checker(la):
    c, m, pf, pg = problem(la)
    seed, nit, C_ = 3, 5, S.N_CHAINS
    ref, og = S.term(m), S.prior_term(c, np.float64)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=C_, tau=m.tau, gamma=m.gamma, seed=seed)
    try:
        smp.set_state(m.x0)
        x = m.x0.astype(np.float64)
        for it in range(1, nit + 1):
            smp.step(1)
            x = P.myula_step(ref, og, x, m.tau, m.gamma, O.philox_normals(seed, it - 1, np.arange(C_), *c.shape).astype(np.float64))
            got = smp.get_state().cpu().numpy()
            e = X.rel(got, x)
            print(f"Philox trajectory step {it}: rel {e:.3e}, worst pixel {S.worst(got, x)[0]:.3e} ({smp.kernel_name})")
            assert e <= STEP_TOL * it, (it, e)
    finally:
        smp.close()


# ------------------------------------------------------------------ 8. refusals
def myula_config(la, shape, data, prior, options=None, **fields):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    prob = _Problem(shape, data, prior, options=options)
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
        assert prob.c.data_kind == _capi.DATA_SENSE and prob.c.kh == c.n_coils
        for create in (lambda h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h))):
            hnd = C.c_void_p()
            rc = create(hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == LMC_E_UNSUPPORTED and "SENSE" in msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, stream)
        assert rc == LMC_E_UNSUPPORTED and "SENSE" in last_error(), (fields, rc, last_error())
    # the samplers and calls without a form of the term
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "LMC_DATA_SENSE" in last_error() and "Metropolis" in last_error() and not hnd.value, (rc, last_error())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "LMC_DATA_SENSE" in last_error() and "implicit step" in last_error() and not hnd.value, (rc, last_error())
    rc = lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 0, 0, None, stream)
    assert rc == LMC_E_UNSUPPORTED and "LMC_DATA_SENSE" in last_error() and "diagonal in neither" in last_error(), (rc, last_error())
    g = _capi.lmc_sgs_config()
    g.struct_size = C.sizeof(_capi.lmc_sgs_config)
    g.problem = prob.c
    g.n_chains, g.rho, g.tau, g.gamma, g.epsg, g.n_inner, g.thin = 2, 1.0, 0.1, X.GAMMA, 1.0, 1, 1
    rc = lib.lmc_sgs_create(C.byref(g), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "LMC_DATA_SENSE" in last_error() and "closed-form draw" in last_error() and not hnd.value, (rc, last_error())
    vt = la.VectorialTV(shape, 2, sigma=0.3).prior_descriptor()
    prob_v, _ = myula_config(la, shape, pf.descriptor(), vt, options={"multichannel": True})
    mc = _capi.lmc_mch_config()
    mc.struct_size = C.sizeof(_capi.lmc_mch_config)
    mc.problem = prob_v.c
    mc.n_channels, mc.n_chains, mc.tau, mc.gamma, mc.epsg, mc.thin = 2, 2, 1e-3, X.GAMMA, 1.0, 1
    rc = lib.lmc_mch_create(C.byref(mc), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "data_kind 20" in last_error() and not hnd.value, (rc, last_error())
    # fields the kind does not read must be empty; the coil count
    keep = np.ones(4, dtype=np.float32)
    for fields in (dict(mask_dev=x.data_ptr()), dict(h_host=_dev.fptr(keep)), dict(kw=3), dict(oy=1), dict(ox=1), dict(psf_kh=3), dict(psf_kw=3),
                   dict(psf_oy=1), dict(psf_ox=1), dict(y_dev=None), dict(kh=0), dict(kh=-1), dict(kh=33)):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_INVALID and last_error() and not hnd.value, (fields, rc, last_error())
    for fields in (dict(H=12, W=16), dict(H=16, W=4), dict(H=2048, W=16)):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_UNSUPPORTED and "powers of two" in last_error() and not hnd.value, (fields, rc, last_error())
    # the stateless operator
    H, W, nc = shape[0], shape[1], c.n_coils
    head = _dev.to_dev(pf.Op.descriptor())
    ksp = torch.zeros((2, nc, H, W, 2), dtype=torch.float32, device="cuda")
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(ksp), 2, H, W, nc, 0, stream) == 0, last_error()
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(ksp), _dev.ptr(out), 2, H, W, nc, 1, stream) == 0, last_error()
    assert lib.lmc_sense_apply(None, _dev.ptr(x), _dev.ptr(ksp), 2, H, W, nc, 0, stream) == LMC_E_INVALID and last_error()
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(x), 2, H, W, nc, 0, stream) == LMC_E_INVALID
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(ksp), 0, H, W, nc, 0, stream) == LMC_E_INVALID
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(ksp), 2, H, W, 0, 0, stream) == LMC_E_INVALID
    assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(ksp), 2, H, W, 33, 0, stream) == LMC_E_INVALID
    for hh, ww in ((12, 16), (16, 4), (2048, 16)):
        assert lib.lmc_sense_apply(_dev.ptr(head), _dev.ptr(x), _dev.ptr(ksp), 2, hh, ww, nc, 0, stream) == LMC_E_UNSUPPORTED and "powers of two" in last_error()
    # what is not refused: the problem as it stands (iterations_per_launch is ignored), a forced variant of the prior launch
    for fields in (dict(), dict(iterations_per_launch=2), dict(step_variant=1)):
        prob_ok, cfg_ok = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert lib.lmc_myula_create(C.byref(cfg_ok), C.byref(hnd)) == 0, last_error()
        assert lib.lmc_sampler_step(hnd, 1, None, stream) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
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
        la.SplitGibbsSampler(pf, pg, shape, rho=1.0, tau=0.1, gamma=X.GAMMA, n_chains=2)
    with pytest.raises(NotImplementedError):
        la.sgs_xstep(pf, m.x0, 1.0)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.VectorialTV(shape, 2, sigma=0.3), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=1e-4), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=3, warm=True), shape, **kw)
    with pytest.raises(NotImplementedError):
        la.MYULASampler(pf, la.TV(shape, sigma=0.3, niter=3), shape, tv_warm=True, **kw)
    with pytest.raises(NotImplementedError):
        la.SKROCKSampler(pf, la.TV(shape, sigma=0.3, niter=10, rtol=1e-4), shape, n_stages=3, **kw)
    with pytest.raises(NotImplementedError):
        pf.prox(m.x0, 0.5)
    la.MYULASampler(pf, pg, shape, **kw).close()
    la.SKROCKSampler(pf, pg, shape, n_stages=3, **kw).close()
