"""Per-pixel parity of the non-convex data terms of L2_ncvx_tv (MC-TV isotropic and anisotropic, ME-TV) against float64: max |got - ref64| over EVERY
chain and pixel within max(3 e32, 2 ulp32(max |ref64|)), e32 the larger error of two float32 replays of the reference (tests/_ncvx_pixel.py: the
dtype-generic restatement of the term, the two weightings, the conditions on the inputs, the cases; tests/test_ncvx_pixel_reference.py shows on the CPU
which planted faults of the stencil the bound rejects and the rel-L2 norms of tests/test_gpu_ncvx.py accept).

The cases (`_ncvx_pixel.CASES`, two chains, each at the configured weight lamda = 0.3 and at the prominent one tau lamda = 1, or tau lamda / gamma = 1 for
ME-TV): the tile, split, point, block, rows and pipe kernels with `variant=` forced and the exact `kernel_name` asserted -- MC-TV isotropic and anisotropic
per pixel in the tile, split and point kernels, through the rolling window of the fused Haar block kernel and as `mc_tv_add_kernel` after the block kernel
for l1 / l2, row by row in the pipe kernel (lane seams, unaligned widths, column strips, K = 2, 6, 8, 9, the chain of two launches, the warm dual, other
taps, the anisotropic prior); ME-TV with the inner prox chunked in the tile kernel (10, 17, 18, 50 dual iterations), in the split kernel (10) and as a chain
of five launches of the pipe kernel (50), and as a ready-made gradient array in the row kernel.  What a variant does not cover must refuse with
LMC_E_UNSUPPORTED: the two-team pipe layout with either term, the row kernel with MC-TV, and -- because a forced variant runs the inner prox too
(`me_tv_prox`) -- the split kernel with 50 inner iterations and the row kernel forced with ME-TV (the row cases therefore run under the library's own
choice and assert that it IS the row kernel).  Then `L2_ncvx_tv.prox`: the pre-steps ulpda_ncvx_rhs_kernel and ulpda_me_rhs_kernel with the closed-form
solve (identity, mask), with blur A in front of 50 CG iterations, and inside ULPDA sampler iterations (state and both dual components); the value
`L2_ncvx_tv.__call__` over the 32 x 64 tile of the energy kernels; and the refusals of the Poisson and weighted data terms and of ULPDA without a data
term.

Measured on an MI355X (all 293 tests pass; 188 step cases run and 10 refuse as asserted; the whole file takes 5 s, 2 s of it the references): the largest
err / e32 of each family over its cases and iterations, and where it sat; the bound is at ratio 3.  No family has its worst pixel at an edge or seam, and
the largest ratio off the interior (last) is below the interior's everywhere but in the pointwise prox, whose worst pixel happens to lie in the first row.

    family                    verdicts  largest err / e32   case, region                                                largest off the interior
    tile                           120  1.26                (66, 67) ME-TV 50 prominent, interior (err 4.8e-5)          0.61 last row, (3, 5) aniso
    split                           40  0.87                (5, 65) ME-TV 10 prominent, second iteration, interior      0.64 column seam 64
    point                           32  0.48                (33, 65) aniso l2 blur B configured, interior               0.40 column seam 64
    block                           52  1.41                (8, 8) MC l1 identity + mc_tv_add, interior (err 2.5e-5)    1.11 column seam 32, (16, 72) aniso Haar mask
    rows                            36  0.91                (9, 4) ME-TV 10 l1 prominent, interior (err 1.2e-5)         0.72 last column
    pipe                            98  1.46                (6, 264) ME-TV 50 prominent, interior (err 5.3e-5)          0.52 lane seam 64, (6, 132) MC
    prox, identity / mask           48  1.24                (17, 67) ME-TV 50 identity prominent, first row (3.3e-5)    1.24 first row
    prox, blur A + 50 CG            12  0.91                (40, 64) ME-TV 50 configured, row seam 16 (err 1.2e-4)      0.91 row seam 16
    ULPDA iteration, state          16  1.07                (17, 67) MC blur A configured, second iteration, interior   (no edge or seam pixel was the worst)
    ULPDA iteration, dual           32  1.75                (17, 67) MC blur A prominent, interior (err 1.8e-5)         0.62 row seam 16

The value: largest |got - float64| / tolerance 0.061 over the 24 shapes ((1, 3), both kinds; 0.017 at most on the others): the device sums its float32
envelopes in double, as the replay does, and both sit at 1e-9 to 6e-8 relative, under the floor of 1e-6.  No test exposed a fault; the library is unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import _ncvx_pixel as N
import _pixel as X

pytestmark = pytest.mark.gpu
LMC_E_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def f64(a):
    return None if a is None else np.array(a, dtype=np.float64)      # (the same numbers; the reference's arrays are read-only)


def ncvx_term(la, shape, nc, niter, lam, Op, b, sigma, solve_iters=None):
    """`la.L2_ncvx_tv` of one kind over operator `Op` (None: the identity).  `niter` of the class counts the inner prox of ME-TV AND the CG iterations of
    `prox`; `solve_iters` sets the latter for MC-TV."""
    if Op is None:
        Op = la.Identity(shape[0] * shape[1])
    kw = dict(dims=shape, Op=Op, b=f64(b).ravel(), sigma=sigma, lamda=lam, gamma=N.CFG_GAMMA, warm=False)
    if nc == "me":
        assert solve_iters in (None, niter)
        return la.L2_ncvx_tv(isotropic=True, niter=niter, rtol=0.0, **kw)
    return la.L2_ncvx_tv(Op2=la.Gradient(shape), isotropic=nc == "mc", niter=solve_iters or 10, **kw)


def device_terms(la, n):
    """The library's data term with the non-convex term and the prior of case `n`, from the float32 numbers of `_ncvx_pixel.problem`."""
    c, m, shape = n.base, N.problem(n), n.base.shape
    if m.h is not None:
        Op = la.Convolve2D(shape, f64(m.h), offset=m.offset)
    elif m.mask is not None:
        Op = la.Diagonal(f64(m.mask), dims=shape)
    else:
        Op = None
    pf = ncvx_term(la, shape, n.nc, n.niter, N.lam_of(n, m.tau), Op, m.y, m.sigma_f)
    w = X.weight(c)
    if c.prior in ("tv", "aniso"):
        pg = la.TV(shape, sigma=w, niter=c.K + (1 if c.lagged else 0), lagged_output=c.lagged, warm=c.mode == "warm", isotropic=c.prior == "tv")
    elif c.prior == "l1":
        pg = la.L1(sigma=w)
    elif c.prior == "l2":
        pg = la.L2(sigma=w, dims=shape)
    elif c.prior == "haar":
        pg = la.WaveletL1(shape, sigma=w)
    else:
        pg = None
    return pf, pg


_RUNS = {}


def run(la, n):
    """The device run of case `n`, once per process: {"states": the state after each iteration, "kernel": its name} or {"refused": status}."""
    key = N.case_id(n)
    if key in _RUNS:
        return _RUNS[key]
    c, m, stages = n.base, N.problem(n), N.reference(n)
    pf, pg = device_terms(la, n)
    smp = None
    try:
        smp = la.MYULASampler(pf, pg, c.shape, noise="injected", n_chains=N.N_CHAINS, tau=m.tau, gamma=m.gamma, variant=c.variant)
        states = []
        for it, st in enumerate(stages):
            if st.start is not None:
                smp.set_state(f64(st.start))
            smp.step(1, noise=f64(m.noise[it:it + 1]))
            states.append(smp.get_state().cpu().numpy())
        out = {"states": states, "kernel": smp.kernel_name}
    except la.LMCError as err:
        out = {"refused": err.code, "message": str(err)}
    finally:
        if smp is not None:
            smp.close()
    _RUNS[key] = out
    return out


def _fail_on(verdicts):
    bad = [v.message for v in verdicts if not v.ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", N.CASES, ids=N.IDS)
def test_every_pixel_of_the_step_with_the_term_within_the_reference_bound(la, n):
    out = run(la, n)
    if n.base.kernel is None:
        assert out.get("refused") == LMC_E_UNSUPPORTED, out
        return
    assert "refused" not in out, out
    assert out["kernel"] == n.base.kernel, (out["kernel"], n.base.kernel)
    stages = N.reference(n)
    assert len(stages) == len(out["states"])
    _fail_on([X.check(n.base, it, got, st) for (it, st), got in zip(enumerate(stages), out["states"])])


@pytest.mark.parametrize("c", N.P_CASES, ids=N.P_IDS)
def test_prox_prestep_and_pointwise_solve_per_pixel(la, c):
    """`L2_ncvx_tv.prox` with the identity and with a mask: ulpda_ncvx_rhs_kernel / ulpda_me_rhs_kernel, then the closed-form solve."""
    m, st = N.p_problem(c), N.p_reference(c)
    Op = la.Diagonal(f64(m.mask), dims=c.shape) if m.mask is not None else None
    pf = ncvx_term(la, c.shape, c.nc, c.niter, N.p_lam(c), Op, m.b, N.P_SIGMA)
    got = np.asarray(pf.prox(f64(m.x0).reshape(N.N_CHAINS, -1), N.P_TAU)).reshape((N.N_CHAINS,) + c.shape)
    _fail_on([X.check(c, 0, got, st)])


@pytest.mark.parametrize("c", N.S_CASES, ids=N.S_IDS)
def test_prox_with_a_blur_and_one_ulpda_iteration_per_pixel(la, c):
    """The pre-steps in front of the converged solve (50 CG iterations, tolerance off): `L2_ncvx_tv.prox` with blur A, and ULPDA sampler iterations
    (restart from ref64 after the first) with the identity and with blur A; state and dual against the bounds of tests/_ulpda_pixel.py."""
    m, stages, shape = N.s_problem(c), N.s_reference(c), c.shape
    Op = la.Convolve2D(shape, f64(m.h), offset=m.offset) if m.h is not None else None
    pf = ncvx_term(la, shape, c.nc, c.niter, N.s_lam(c), Op, m.b, N.U.SIGMA_F, solve_iters=N.U.CG_ITERS if m.h is not None else None)
    verdicts = []
    if c.entry == "prox":
        prev = la.set_cg_tolerance(0.0)
        try:
            got = np.asarray(pf.prox(f64(m.x0).reshape(N.N_CHAINS, -1), N.S_TAU)).reshape((N.N_CHAINS,) + shape)
        finally:
            la.set_cg_tolerance(prev)
        verdicts += N.s_check(c, 0, got, None, stages[0])
    else:
        smp = la.ULPDASampler(pf, la.L21(ndim=2, sigma=N.U.RADIUS), la.Gradient(shape), shape, n_chains=N.N_CHAINS, tau=N.S_TAU, mu=N.S_MU, theta=N.S_THETA,
                              gfirst=False, noise="injected", implicit_tol=-1)
        try:
            for it, st in enumerate(stages):
                smp.set_state(f64(st.start_x))       # (also xhat = x)
                smp.set_dual(f64(st.start_y))
                smp.step(1, noise=f64(m.noise[it:it + 1]))
                verdicts += N.s_check(c, it, smp.get_state().cpu().numpy(), smp.get_dual().cpu().numpy(), st)
            assert smp.kernel_name == "ulpda (multi-kernel)", smp.kernel_name
        finally:
            smp.close()
    _fail_on(verdicts)


@pytest.mark.parametrize("c", N.E_CASES, ids=N.E_IDS)
def test_value_per_chain_at_the_prominent_weight(la, c):
    """`L2_ncvx_tv.__call__` against the float64 value on the float32 inputs: within 3 x the error of the float32 replay of the per-pixel envelope summed
    in float64, floor 1e-6 relative.  Measured on an MI355X: err / tolerance at most 0.061 ((1, 3)), relative error 1.5e-9 to 6.1e-8."""
    h, off, y, x0 = N.e_problem(c.shape)
    pf = ncvx_term(la, c.shape, c.nc, 0, N.e_lam(), la.Convolve2D(c.shape, f64(h), offset=off), y, 1 / X.SIGMA ** 2)
    got = np.atleast_1d(np.asarray(pf(f64(x0)), dtype=np.float64))
    want, tol, e32 = N.e_reference(c)
    err = np.abs(got - want)
    print(f"energy {c.tag}: err / tol {np.max(err / tol):.3f}, rel err {np.max(err / np.abs(want)):.2e}, replay rel err {np.max(e32 / np.abs(want)):.2e}")
    assert got.shape == want.shape and np.all(err <= tol), (got, want, tol)


def _myula_config(la, shape, data, prior, **fields):
    from lmc_atomi_amd import _capi
    from lmc_atomi_amd.proximal import _Problem
    prob = _Problem(shape, data, prior)
    for k, v in fields.items():
        setattr(prob.c, k, v)
    cfg = _capi.lmc_myula_config()
    cfg.struct_size = C.sizeof(_capi.lmc_myula_config)
    cfg.problem = prob.c
    cfg.n_chains = N.N_CHAINS
    cfg.tau, cfg.gamma, cfg.epsg = 1e-3, 0.5, 1.0
    cfg.noise_mode = _capi.NOISE_PHILOX
    cfg.thin = 1
    return prob, cfg


@pytest.mark.parametrize("kind", ["mc", "mca", "me"])
def test_data_terms_without_a_non_convex_form_refuse(la, kind):
    """The Poisson and the weighted Gaussian data term with a non-convex term, and ULPDA with the term and no data term: LMC_E_UNSUPPORTED, no handle."""
    from lmc_atomi_amd import _capi, _dev
    lib = _dev.lib()
    shape = (17, 67)
    rng = np.random.default_rng(3)
    y = rng.uniform(1.0, 30.0, shape)
    fields = {"mc": dict(ncvx_kind=_capi.NCVX_MC_TV), "mca": dict(ncvx_kind=_capi.NCVX_MC_TV_ANISO), "me": dict(ncvx_kind=_capi.NCVX_ME_TV, ncvx_niter=10)}[kind]
    fields.update(ncvx_gamma=N.CFG_GAMMA, ncvx_lambda=N.CFG_LAMBDA)
    H = la.Convolve2D(shape, X.BLURS["A"][0], offset=X.BLURS["A"][1])
    prior = la.TV(shape, sigma=0.3, niter=10).prior_descriptor()
    for pf in (la.Poisson(H, y, 2.0, sigma=1.0), la.L2(Op=H, b=y, sigma=1.0, weights=np.ones(shape), dims=shape)):
        prob, cfg = _myula_config(la, shape, pf.descriptor(), prior, **fields)
        hnd = C.c_void_p()
        rc = lib.lmc_myula_create(C.byref(cfg), C.byref(hnd))
        msg = lib.lmc_last_error().decode()
        if rc == 0:
            lib.lmc_sampler_destroy(hnd)
        assert rc == LMC_E_UNSUPPORTED and msg and not hnd.value, (type(pf).__name__, rc, msg)
    prob, _ = _myula_config(la, shape, None, prior, **fields)      # (prior_kind TV_ISO: the dual ball of ULPDA)
    u = _capi.lmc_ulpda_config()
    u.struct_size = C.sizeof(_capi.lmc_ulpda_config)
    u.problem = prob.c
    u.n_chains, u.tau, u.mu, u.theta, u.cg_niter, u.thin = N.N_CHAINS, 0.1, 0.1, 1.0, 5, 1
    hnd = C.c_void_p()
    rc = lib.lmc_ulpda_create(C.byref(u), C.byref(hnd))
    msg = lib.lmc_last_error().decode()
    if rc == 0:
        lib.lmc_sampler_destroy(hnd)
    assert rc == LMC_E_UNSUPPORTED and "non-convex" in msg and not hnd.value, (rc, msg)
