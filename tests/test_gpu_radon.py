"""GPU parity of the parallel-beam Radon operator (`la.Radon`, LMC_DATA_RADON .. LMC_DATA_HUBER_RADON in include/lmc_atomi.h) against the references of
tests/_radon_ref.py: the operator and its adjoint per output against the derived bound, adjointness, more than 65535 images, one MYULA step per pixel
for the four data terms and the priors that take another kernel in the middle launch, the Philox path, chain sharding, a trajectory, SK-ROCK, SAPG,
the energies, and the refusals of the C ABI and of the Python surface.

Operator: per output |got - ref64| <= 2^-24 ((n + 2) S_w + 2 S_1), exactly 0 where no weight is positive (tests/_radon_ref.py).  Steps: per pixel
max(3 e32, 2 ulp32(max |ref64|)), e32 measured on the checker's float32 replay (tests/_pixel.py).  Trajectories: rel-L2 1e-5 x (step index);
energies: rtol 5e-5."""
import ctypes as C

import numpy as np
import pytest

import _many as M
import _pixel as X
import _poisson_ref as P
import _radon_ref as R
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


def within_operator(what, got, ref):
    ratio, stray = R.worst_ratio(got, ref)
    print(f"operator {what}: worst err / bound {ratio:.3f}; largest value where no weight is positive {stray:.1e}")
    assert ratio <= 1.0 and stray == 0.0, (what, ratio, stray)
    return ratio


def within(what, got, ref64, bound, e32):
    err, where = R.worst(got, ref64)
    print(f"pixel {what}: err {err:.3e} at {where}, e32 {e32:.3e}, bound {bound:.3e}, err / bound {err / bound:.2f}")
    assert err <= bound, (what, err, bound, where)
    return err


# ------------------------------------------------------------------ 1. the operator, both directions
@pytest.mark.parametrize("name", R.OP_IDS)
def test_operator_and_adjoint_per_output(la, name):
    c = R.OP_CASES[R.OP_IDS.index(name)]
    op = la.Radon(c.shape, c.angles, c.n_det)
    fwd, adj = R.op_references(name)
    assert op.sino_shape == (len(c.angles), R.case_n_det(c)) and op.shape == (fwd.ref64.shape[1], adj.ref64.shape[1])
    got_f = op.matvec(fwd.x)
    got_a = op.rmatvec(adj.x)
    assert got_f.shape == fwd.ref64.shape and got_f.dtype == np.float32 and got_a.shape == adj.ref64.shape
    within_operator(f"{name} A", got_f, fwd)
    within_operator(f"{name} A^T", got_a, adj)
    # image- and sinogram-shaped operands, and the pylops protocol on flat vectors: @, .H
    shaped = op.matvec(fwd.x.reshape((R.N_IMG,) + c.shape))
    assert np.array_equal(np.asarray(shaped).reshape(got_f.shape), np.asarray(got_f))
    assert np.array_equal(np.asarray(op.rmatvec(adj.x.reshape((R.N_IMG,) + op.sino_shape))).reshape(got_a.shape), np.asarray(got_a))
    flat = op @ fwd.x[0]
    assert flat.shape == (op.shape[0],) and np.array_equal(flat, np.asarray(got_f)[0])
    back = op.H @ adj.x[1]
    assert back.shape == (op.shape[1],) and np.array_equal(back, np.asarray(got_a)[1])
    # deterministic: a second run gives the same bits
    assert np.array_equal(np.asarray(op.matvec(fwd.x)), np.asarray(got_f)) and np.array_equal(np.asarray(op.rmatvec(adj.x)), np.asarray(got_a))


@pytest.mark.parametrize("name", R.OP_IDS)
def test_adjointness_from_the_device_outputs(la, name):
    """<A x, r> = <x, A^T r> summed in float64: each side is off by at most its bound per output times the magnitude of the other operand there."""
    c = R.OP_CASES[R.OP_IDS.index(name)]
    op = la.Radon(c.shape, c.angles, c.n_det)
    fwd, adj = R.op_references(name)
    x, r = fwd.x.astype(np.float64), adj.x.astype(np.float64)
    ax = np.asarray(op.matvec(fwd.x), dtype=np.float64)
    atr = np.asarray(op.rmatvec(adj.x), dtype=np.float64)
    lhs, rhs = float(np.sum(ax * r)), float(np.sum(x * atr))
    tol = float(np.sum(fwd.bound * np.abs(r)) + np.sum(adj.bound * np.abs(x)))
    print(f"adjointness {name}: <Ax, r> = {lhs:.9e}, <x, A^T r> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


def test_more_images_than_a_grid_dimension_holds(la):
    """70000 images of 4 x 4 at 3 angles: image c is pattern c % 7, so an image index that wraps or loses its chunk shows as another pattern."""
    n, shape, angles = 70000, (4, 4), [0.2, 1.1, 2.5]
    ref = R.RadonRef(shape, angles)
    op = la.Radon(shape, angles)
    base = X.f32(M.patterns(shape, seed=4)).reshape(M.P, -1)
    sino = X.f32(np.random.default_rng(8).standard_normal((M.P, op.shape[0])) * 30.0)
    for what, fn, operand, adjoint in (("A", op.matvec, base, False), ("A^T", op.rmatvec, sino, True)):
        M64 = ref.A.T if adjoint else ref.A
        r64 = operand.astype(np.float64) @ M64.T
        bound = R.operator_bound(ref.A, operand, adjoint)
        got = fn(M.tile_dev(operand, n)).cpu().numpy()
        assert got.shape == (n, r64.shape[1])
        k = M.tile_index(n)
        d = np.abs(got.astype(np.float64) - r64[k])
        d = np.where(np.isfinite(d), d, np.inf)
        ratio = d / np.maximum(bound[k], 1e-300)
        w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print(f"70000 images {what}: worst err / bound {ratio[w]:.3f} at image {w[0]} (pattern {w[0] % M.P})")
        assert ratio[w] <= 1.0, (what, w, d[w], bound[k][w])


# ------------------------------------------------------------------ 2. one MYULA step per pixel ("restart" mode)
def device_terms(la, c, m):
    op = la.Radon(c.shape, R.STEP_ANGLES)
    assert op.sino_shape == m.op.sino_shape
    if c.term == "pois":
        pf = la.Poisson(op, m.y, m.aux, sigma=m.sigma_f)
    elif c.term == "wl2":
        pf = la.L2(Op=op, b=m.y, sigma=m.sigma_f, weights=m.aux)
    elif c.term == "hub":
        pf = la.HuberLoss(op, m.y, m.aux, sigma=m.sigma_f)
    else:
        pf = la.L2(Op=op, b=m.y, sigma=m.sigma_f)
    if c.prior == "tv":
        pg = la.TV(c.shape, sigma=m.weight, niter=c.K, bounds=c.box)
    elif c.prior == "l1":
        pg = la.L1(sigma=m.weight)
    else:
        pg = None
    return pf, pg


def problem_of(la, name):
    c = R.STEP_CASES[R.STEP_IDS.index(name)]
    m = R.step_problem(name)
    return (c, m) + device_terms(la, c, m)


MIDDLE_KERNEL = {"l2-tv10-pipe": ("myula_step_pipe_kernel",), "l2-tv10": ("myula_step_tile_kernel", "myula_step_split_kernel"),
                 "pois-tvpos": ("myula_step_tile_box_kernel",)}


@pytest.mark.parametrize("name", [n for n in R.STEP_IDS if not n.endswith("-grad")])
def test_myula_step_per_pixel(la, name):
    c, m, pf, pg = problem_of(la, name)
    stages = R.step_reference(name)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=R.N_IMG, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        for it, st in enumerate(stages):
            smp.set_state(st.start)
            smp.step(1, noise=m.noise[it:it + 1])
            got = smp.get_state().cpu().numpy()
            within(f"{name} it {it} ({smp.kernel_name})", got, st.ref64, st.bound, st.e32)
        if name in MIDDLE_KERNEL:
            assert smp.kernel_name in MIDDLE_KERNEL[name], smp.kernel_name
    finally:
        smp.close()


@pytest.mark.parametrize("term", R.TERMS)
def test_gradient_alone_is_the_overwrite_form(la, term):
    """No prox and no noise (b = s = 0): the adjoint launch writes a x - t sigma A^T rho(A x) alone."""
    name = f"{term}-grad"
    c, m, pf, _ = problem_of(la, name)
    st = R.step_reference(name)[0]
    got = pf.grad(st.start)
    assert got.shape == st.start.shape
    within(name, got, st.ref64, st.bound, st.e32)
    assert pf.grad_lipschitz() == pytest.approx(R.data_term(c, m, np.float64).grad_lipschitz() if term != "l2" else m.sigma_f * m.op.norm2_bound(), rel=1e-6)


# ------------------------------------------------------------------ 3. Philox, sharding, a trajectory
def run_philox(la, pf, pg, shape, x0, n_chains, chain_offset, seed, nit, m):
    smp = la.MYULASampler(pf, pg, shape, n_chains=n_chains, chain_offset=chain_offset, tau=m.tau, gamma=m.gamma, seed=seed)
    try:
        smp.set_state(x0)
        smp.step(nit)
        return smp.get_state().cpu().numpy(), smp.kernel_name
    finally:
        smp.close()


def test_philox_path_and_chain_sharding_give_equal_bits(la):
    """The noise of a chain depends on its global id only: four chains on one sampler are the chains of two samplers of two (chain_offset 0 and 2);
    and the first step is the checker's step with the checker's Philox field."""
    c, m, pf, pg = problem_of(la, "pois-tvpos")
    x0 = np.concatenate([m.x0, m.x0[:1] + 1.0])
    seed = 9
    want, _ = run_philox(la, pf, pg, c.shape, x0, 4, 0, seed, 3, m)
    assert np.isfinite(want).all() and not np.array_equal(want, x0)
    again, _ = run_philox(la, pf, pg, c.shape, x0, 4, 0, seed, 3, m)
    assert np.array_equal(again, want), "two runs of the same sampler differ: a launch is not deterministic"
    for off in (0, 2):
        part, _ = run_philox(la, pf, pg, c.shape, x0[off:off + 2], 2, off, seed, 3, m)
        np.testing.assert_array_equal(part, want[off:off + 2])
    one, kernel = run_philox(la, pf, pg, c.shape, x0, 4, 0, seed, 1, m)
    xi = O.philox_normals(seed, 0, np.arange(4), *c.shape).astype(np.float64)
    ref = P.myula_step(R.data_term(c, m, np.float64), R.prior_term(c, m, np.float64), x0.astype(np.float64), m.tau, m.gamma, xi)
    e = X.rel(one, ref)
    print(f"Philox step: rel {e:.3e} ({kernel})")
    assert e <= STEP_TOL, e


def test_trajectory_of_five_steps(la):
    c, m, pf, pg = problem_of(la, "wl2-tv10")
    nit = 5
    noise = X.f32(np.random.default_rng(21).standard_normal((nit, R.N_IMG) + c.shape))
    ref, og = R.data_term(c, m, np.float64), R.prior_term(c, m, np.float64)
    smp = la.MYULASampler(pf, pg, c.shape, n_chains=R.N_IMG, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        smp.set_state(m.x0)
        x = m.x0.astype(np.float64)
        for it in range(nit):
            x = P.myula_step(ref, og, x, m.tau, m.gamma, noise[it].astype(np.float64))
            smp.step(1, noise=noise[it:it + 1])
            e = X.rel(smp.get_state().cpu().numpy(), x)
            print(f"trajectory step {it + 1}: rel {e:.3e} ({smp.kernel_name})")
            assert e <= STEP_TOL * (it + 1), (it, e)
    finally:
        smp.close()


# ------------------------------------------------------------------ 4. SK-ROCK, SAPG
def test_skrock_matches_the_restated_recursion(la):
    s, eta = 3, 0.05
    c, m, pf, pg = problem_of(la, "hub-tv10")
    ref, og = R.data_term(c, m, np.float64), R.prior_term(c, m, np.float64)
    Z = np.random.default_rng(4).standard_normal((1,) + m.x0.shape)
    smp = la.SKROCKSampler(pf, pg, c.shape, n_stages=s, eta=eta, n_chains=R.N_IMG, tau=m.tau, gamma=m.gamma, noise="injected")
    try:
        smp.set_state(m.x0)
        x = P.skrock_iteration(ref, og, m.x0.astype(np.float64), X.f32(Z[0]).astype(np.float64), m.tau, m.gamma, s, eta)
        smp.step(1, noise=Z)
        e = X.rel(smp.get_state().cpu().numpy(), x)
        print(f"SK-ROCK iteration: rel {e:.3e} ({smp.kernel_name})")
        assert e <= STEP_TOL, e
    finally:
        smp.close()


def test_sapg_follows_the_host_update_on_the_device_statistic(la):
    c, m, pf, pg = problem_of(la, "l2-tv10")
    n_updates, bounds = 5, (1e-3, 1e2)
    kw = dict(step_scale=0.02, step_exponent=0.8)
    res = la.EstimatePriorWeight(pf, pg, m.x0, m.tau, m.gamma, n_updates, bounds, theta0=m.weight, seed=5, n_chains=R.N_IMG, dims=c.shape, **kw)
    dim, k = la.sapg_dimension(pg, c.shape)
    trace = [m.weight]
    for n in range(n_updates):
        trace.append(la.sapg_update(trace[-1], float(res.stat_trace[n]), n, dim, k, theta_bounds=bounds, **kw))
    trace = np.array(trace)
    print(f"SAPG theta trace {res.theta_trace} (host replay {trace}); statistic {res.stat_trace}")
    assert res.theta_trace.shape == (n_updates + 1,) and res.theta_trace[0] == m.weight
    assert np.all(np.isfinite(res.stat_trace)) and np.all(res.stat_trace > 0)
    assert np.all((trace[1:] > bounds[0]) & (trace[1:] < bounds[1])) and not np.allclose(trace[1:], m.weight), "the updates move theta and none is clamped"
    assert np.max(np.abs(res.theta_trace - trace) / trace) <= 1e-12, (res.theta_trace, trace)


# ------------------------------------------------------------------ 5. energies
def f_reference(c, m, x):
    if c.term == "l2":
        return R.l2_value(m.op, m.y, m.sigma_f, x)
    return np.asarray(R.data_term(c, m, np.float64)(np.asarray(x, dtype=np.float64)))


@pytest.mark.parametrize("name", ["l2-tv10", "pois-tvpos", "wl2-tv10", "hub-tv10"])
def test_energies_match_float64_and_repeat_bit_for_bit(la, name):
    from lmc_atomi_amd.proximal import _Problem
    c, m, pf, pg = problem_of(la, name)
    want = f_reference(c, m, m.x0)
    got = np.asarray(pf(m.x0))                                       # __call__ of the term
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
    res = la.MoreauYosidaUnadjustedLangevin(pf, pg, m.x0, tau=m.tau, gamma=m.gamma, niter=2, seed=3, n_chains=R.N_IMG, dims=c.shape)
    state = res.state.cpu().numpy()
    ef = res.energy_f.cpu().numpy()                                  # lmc_sampler_energies
    want_s = f_reference(c, m, state.reshape((R.N_IMG,) + c.shape))
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


@pytest.mark.parametrize("name", ["l2-tv10", "pois-tvpos", "wl2-tv10", "hub-tv10"])
def test_c_abi_refusals(la, name):
    import torch
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    c, m, pf, _ = problem_of(la, name)
    shape = c.shape
    prior = la.TV(shape, sigma=0.3, niter=10).prior_descriptor()
    x = torch.zeros((2,) + shape, dtype=torch.float32, device="cuda")
    out = torch.empty_like(x)
    stream = _dev.stream_ptr(x.device)
    for fields in REFUSED:
        prob, cfg = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert prob.c.data_kind in _capi.RADON_KINDS
        for create in (lambda h: lib.lmc_myula_create(C.byref(cfg), C.byref(h)), lambda h: lib.lmc_skrock_create(C.byref(cfg), 3, 0.05, C.byref(h))):
            hnd = C.c_void_p()
            rc = create(hnd)
            msg = last_error()
            if rc == 0:
                lib.lmc_sampler_destroy(hnd)
            assert rc == LMC_E_UNSUPPORTED and msg and not hnd.value, (fields, rc, msg)
        rc = lib.lmc_fused_eval(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 1.0, 0.1, 0.5, 0.1, stream)
        assert rc == LMC_E_UNSUPPORTED and last_error(), (fields, rc, last_error())
    # the samplers and the entry point without a form of the operator
    prob, cfg = myula_config(la, shape, pf.descriptor(), prior)
    hnd = C.c_void_p()
    rc = lib.lmc_mymala_create(C.byref(cfg), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "Radon" in last_error() and not hnd.value, (rc, last_error())
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = 2, 0.1, 0.1, 1.0, 5, 1
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    assert rc == LMC_E_UNSUPPORTED and "Radon" in last_error() and not hnd.value, (rc, last_error())
    ws = torch.empty(lib.lmc_l2_prox_workspace_bytes(2, *shape), dtype=torch.uint8, device="cuda")
    rc = lib.lmc_l2_prox(C.byref(prob.c), _dev.ptr(x), _dev.ptr(out), 2, 0.5, 5, 0, _dev.ptr(ws), stream)
    assert rc == LMC_E_UNSUPPORTED and "Radon" in last_error(), (rc, last_error())
    # bad geometry, no angles, and the fields the kinds must leave alone
    bad_angle = np.array(R.STEP_ANGLES, dtype=np.float32)
    bad_angle[2] = np.inf
    mask = torch.ones(shape, dtype=torch.float32, device="cuda")
    for fields in (dict(kh=0), dict(kh=1025), dict(kw=0), dict(kw=4097), dict(h_host=None), dict(oy=1), dict(ox=1), dict(psf_kh=3), dict(psf_ox=1),
                   dict(psf_separable=1), dict(mask_dev=mask.data_ptr()), dict(y_dev=None), dict(h_host=_dev.fptr(bad_angle))):
        prob_b, cfg_b = myula_config(la, shape, pf.descriptor(), prior, **fields)
        rc = lib.lmc_myula_create(C.byref(cfg_b), C.byref(hnd))
        assert rc == LMC_E_INVALID and last_error() and not hnd.value, (fields, rc, last_error())
    # what is not refused: the problem as it stands (iterations_per_launch is ignored), every forced variant the middle launch has
    for fields in (dict(), dict(iterations_per_launch=2), dict(step_variant=1)):
        prob_ok, cfg_ok = myula_config(la, shape, pf.descriptor(), prior, **fields)
        assert lib.lmc_myula_create(C.byref(cfg_ok), C.byref(hnd)) == 0, last_error()
        assert lib.lmc_sampler_step(hnd, 1, None, stream) == 0, last_error()
        lib.lmc_sampler_destroy(hnd)
        hnd = C.c_void_p()
    torch.cuda.synchronize()


def test_radon_apply_refuses_bad_arguments(la):
    import torch
    from lmc_atomi_amd import _dev
    lib = _dev.lib()
    ang = np.array([0.1, 1.0, 2.0], dtype=np.float32)
    x = torch.zeros((2, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.empty((2, 3, 14), dtype=torch.float32, device="cuda")
    st = _dev.stream_ptr(x.device)
    call = lambda xp, op_, a, na, nd: lib.lmc_radon_apply(xp, op_, 2, 8, 8, a, na, nd, 0, st)
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(ang), 3, 14) == 0, last_error()
    assert call(_dev.ptr(x), _dev.ptr(x), _dev.fptr(ang), 3, 14) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), None, 3, 14) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(ang), 0, 14) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(ang), 1025, 14) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(ang), 3, 0) == LMC_E_INVALID
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(ang), 3, 4097) == LMC_E_INVALID and last_error()
    nan = np.array([0.1, np.nan, 2.0], dtype=np.float32)
    assert call(_dev.ptr(x), _dev.ptr(out), _dev.fptr(nan), 3, 14) == LMC_E_INVALID
    torch.cuda.synchronize()


def test_python_refusals(la):
    c, m, pf, pg = problem_of(la, "l2-tv10")
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
    la.MYULASampler(pf, pg, shape, **kw).close()
    la.SKROCKSampler(pf, pg, shape, n_stages=3, **kw).close()
    la.MYULASampler(pf, pg, shape, variant="tile", **kw).close()
