"""Per-pixel parity of ULPDA and of its implicit solve against the float64 checker: max |got - ref64| over EVERY chain and pixel within
max(3 e32, floor), for the primal state and both components of the dual (tests/_ulpda_pixel.py: the cases, the two replays, the floors, how truncation
is taken out of the solves; tests/test_ulpda_pixel_reference.py shows on the CPU what the rel-L2, residual-norm and row-maximum criteria of
tests/test_gpu_ulpda.py let through).

Part A: ulpda_dual*, ulpda_rhs*, ulpda_pointwise_prox, ulpda_finish* and ulpda_finish_philox_kernel as finite computations, in their scalar and 4-pixel
forms.  Part B: (I + ts H^T H) u = rhs through `L2.prox` and through a sampler iteration on the five paths of the solver -- Chebyshev by single launches
(general taps; the uniform box), Chebyshev pairs, CG with the fused dot on the row kernel, CG on the general kernels -- and three warm-started sampler
iterations on each Chebyshev path, with the residual per pixel as a second quantity.  Every verdict prints its worst pixel, region and err / e32.

Measured on an MI355X (all 215 cases pass; 1012 verdicts; the whole file takes 7 s): the largest err / e32 of the state, the residual and the dual
(the bound is at 3) -- Part A 1.00 / - / 1.00 with injected noise and with Philox noise alike (at 559 worst pixels the kernels are bit-equal to one of
the two replays); Chebyshev single launches, general taps 0.93 / 0.96 / 1.49; uniform box 1.33 / 1.51 / 1.00; Chebyshev pairs 0.94 / 1.21 / 1.30; CG on
the row kernel 1.16 / 1.17 / -; CG on the general kernels 0.78 / 0.77 / -.  No edge or seam stands apart from the interior (DESIGN section 4.1 has the
table)."""
import numpy as np
import pytest

import _ulpda_pixel as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


def f64(a):
    return None if a is None else np.array(a, dtype=np.float64)      # (the same numbers; the reference's arrays are read-only)


def _fail_on(verdicts):
    bad = [v.message for v in verdicts if not v.ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", U.A_CASES, ids=U.A_IDS)
def test_kernels_around_the_solve(la, c):
    m, stages, shape = U.a_problem(c), U.a_reference(c), c.shape
    if c.data == "identity":
        pf = la.L2(b=f64(m.b), sigma=U.SIGMA_F, dims=shape)
    elif c.data == "mask":
        pf = la.L2(Op=la.Diagonal(f64(m.mask), dims=shape), b=f64(m.b), sigma=U.SIGMA_F, dims=shape)
    else:
        pf = None
    pg = la.L21(ndim=2, sigma=U.RADIUS) if c.prior == "l21" else la.L1(sigma=U.RADIUS)
    smp = la.ULPDASampler(pf, pg, la.Gradient(shape), shape, n_chains=U.N_CHAINS, tau=U.A_TAU, mu=U.A_MU, theta=c.theta, gfirst=c.gfirst, z=f64(m.z),
                          seed=U.SEED, chain_offset=U.CHAIN_OFFSET, noise="philox" if c.mode == "philox" else "injected")      # ((3, 1) included: one column)
    verdicts = []
    try:
        if c.mode == "philox":
            smp.set_state(f64(m.x0))
            smp.set_dual(f64(m.y0))
            smp.step(c.iters)
            verdicts += U.check_stage(c, c.iters - 1, smp.get_state().cpu().numpy(), smp.get_dual().cpu().numpy(), stages[-1])
        else:
            for it, st in enumerate(stages):
                smp.set_state(f64(st.start_x))       # (also xhat = x)
                smp.set_dual(f64(st.start_y))
                smp.step(1, noise=f64(m.noise[it:it + 1]))
                verdicts += U.check_stage(c, it, smp.get_state().cpu().numpy(), smp.get_dual().cpu().numpy(), st)
        assert smp.kernel_name == "ulpda (multi-kernel)", smp.kernel_name
    finally:
        smp.close()
    _fail_on(verdicts)


@pytest.mark.parametrize("c", U.B_CASES, ids=U.B_IDS)
def test_implicit_solve_on_every_path(la, c, monkeypatch):
    m, stages, shape = U.b_problem(c), U.b_reference(c), c.shape
    assert U.expected_path(c) == c.family
    if c.pairs:
        monkeypatch.setenv("LMC_CHEB_PAIR", "2")        # pairs also where the launch is too small for them to pay (read when the sampler is made)
        monkeypatch.setenv("LMC_PAIR_BAND", "32")       # rows per wave pair (read per launch)
    else:
        monkeypatch.delenv("LMC_CHEB_PAIR", raising=False)
        monkeypatch.delenv("LMC_PAIR_BAND", raising=False)
    Op = la.Convolve2D(shape, f64(m.h), offset=m.offset)
    pf = la.L2(Op=Op, b=f64(m.b), sigma=U.SIGMA_F, niter=U.CG_ITERS, warm=c.mode == "warm")
    verdicts = []
    if c.entry == "prox":
        prev = la.set_cg_tolerance(U.CHEB_TOL if c.solver == "cheb" else 0.0)
        try:
            out = np.asarray(pf.prox(f64(m.x0).reshape(U.N_CHAINS, -1), U.B_TAU)).reshape((U.N_CHAINS,) + shape)
        finally:
            la.set_cg_tolerance(prev)
        verdicts += U.check_b(c, 0, out, None, stages[0])
    else:
        smp = la.ULPDASampler(pf, la.L21(ndim=2, sigma=U.RADIUS), la.Gradient(shape), shape, n_chains=U.N_CHAINS, tau=U.B_TAU, mu=U.B_MU, theta=U.B_THETA,
                              gfirst=False, noise="injected" if c.mode == "warm" else "none", implicit_tol=U.CHEB_TOL if c.solver == "cheb" else -1)
        try:
            smp.set_state(f64(m.x0))
            for it, st in enumerate(stages):
                if c.mode == "warm":
                    smp.step(1, noise=f64(m.noise[it:it + 1]))
                else:
                    smp.step(1)
                verdicts += U.check_b(c, it, smp.get_state().cpu().numpy(), smp.get_dual().cpu().numpy(), st)
            assert ("pairs" in smp.kernel_name) == (c.family == "cheb-pairs"), (smp.kernel_name, c.family)
        finally:
            smp.close()
    _fail_on(verdicts)
