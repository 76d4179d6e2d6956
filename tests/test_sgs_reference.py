"""CPU-only: the reference of the split Gibbs sampler (tests/_sgs_ref.py) against what it restates -- the conditional draw against a dense solve, the
two-block Gibbs sampler against the closed form of its stationary law under a Gaussian prior, and the planted faults against the bound of every case of
tests/test_gpu_sgs.py.  numpy only; no device, no library."""
import numpy as np
import pytest

import _fourier_ref as F
import _sgs_ref as S


def dense_problem(shape, seed=0):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    G[rng.random(shape) < 0.4] = 0
    assert (G == 0).any()
    b = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return rng, G, b


# ------------------------------------------------------------------ 1. the conditional draw
@pytest.mark.parametrize("shape", [(4, 6), (8, 8)], ids=["4x6", "8x8"])
def test_spectral_draw_has_the_dense_mean_and_covariance(shape):
    sig, rho = 0.7, 1.3
    rng, G, b = dense_problem(shape)
    n = shape[0] * shape[1]
    Ah, Bh = S.tables(G, b, np.float64)
    E = np.eye(n).reshape((n,) + shape)
    grad = lambda x: F.SpectralRef(G, b, sig).grad(x)                 # the definition on the full plane, not the fold
    hess = np.stack([(grad(e) - grad(0 * e)).ravel() for e in E])
    Q = hess + np.eye(n) / rho ** 2
    draw = lambda z, xi: S.xdraw_spectral(z, xi, Ah, Bh, sig, rho, np.float64)
    z = rng.normal(size=shape)
    mean = draw(z, None)
    want = np.linalg.solve(Q, (z / rho ** 2 - grad(np.zeros(shape))).ravel())
    assert np.max(np.abs(mean.ravel() - want)) <= 1e-12
    Tm = np.stack([(draw(z, e) - mean).ravel() for e in E], axis=1)    # the linear map from xi to x
    assert np.max(np.abs(Tm @ Tm.T - np.linalg.inv(Q))) <= 1e-12
    prox = F.prox_folded(z, G, b, sig, rho ** 2)                       # xi = 0 is prox_{rho^2 f}(z)
    assert np.max(np.abs(prox - mean)) <= 1e-12
    assert np.max(np.abs(draw(z, np.zeros(shape)) - mean)) == 0.0


def test_diagonal_draw_has_the_dense_mean_and_covariance():
    shape, sig, rho = (3, 5), 0.7, 1.3
    rng = np.random.default_rng(2)
    b, w = rng.normal(size=shape), rng.uniform(0.2, 2.0, shape)
    m = (rng.random(shape) < 0.6).astype(np.float64)
    w[0, 0] = 0.0
    z, xi = rng.normal(size=shape), rng.normal(size=shape)
    for bb, ww, mm in ((b, None, None), (b, None, m), (b, w, None), (None, None, None)):
        w1 = np.ones(shape) if ww is None else ww
        m1 = np.ones(shape) if mm is None else mm
        s = sig if bb is not None else 0.0
        q = s * w1 * m1 ** 2 + 1 / rho ** 2                            # Q = Hess f + I / rho^2 is diagonal
        b1 = np.zeros(shape) if bb is None else bb
        want_mean = (z / rho ** 2 + s * w1 * m1 * b1) / q
        assert np.max(np.abs(S.xdraw_diag(z, None, bb, ww, mm, sig, rho, np.float64) - want_mean)) <= 1e-14
        got = S.xdraw_diag(z, xi, bb, ww, mm, sig, rho, np.float64)
        assert np.max(np.abs((got - want_mean) ** 2 - xi ** 2 / q)) <= 1e-13      # T T^T = Q^-1, pixel by pixel


def test_kernel_order_replay_is_the_definition_in_float64_terms():
    """The two float32 replays differ by rounding alone: both are within a few e32 of the float64 reference on every case."""
    for c in S.CASES:
        m = S.problem(c)
        r = S.reference(c)
        for order in ("definition", "kernel"):
            x, z = S.iteration(c, m, m.x0, m.z0, m.noise, np.float32, order)
            assert x.dtype == np.float32 and z.dtype == np.float32
            assert np.max(np.abs(x - r.x64)) <= 3 * r.bx and np.max(np.abs(z - r.z64)) <= 3 * r.bz, (S.case_id(c), order)


# ------------------------------------------------------------------ 2. exactness under a Gaussian prior
def test_two_block_gibbs_has_the_closed_form_marginal():
    x, G = S.gauss_chain_cpu()
    assert x.shape == (S.GAUSS_N,) + S.GAUSS_SHAPE
    assert S.gauss_check(x, G, "reference chain") <= S.GAUSS_SE


@pytest.mark.parametrize("fault", ["noise_over_q", "no_noise"])
def test_the_statistical_check_rejects_a_wrong_draw(fault):
    if fault == "no_noise":
        x, G = S.gauss_chain_cpu()
        x = x.mean(axis=0, keepdims=True) + 0.5 * (x - x.mean(axis=0, keepdims=True))      # half the spread
    else:
        x, G = S.gauss_chain_cpu(fault=fault)
    assert S.gauss_check(x, G, fault) > S.GAUSS_SE


# ------------------------------------------------------------------ 3. planted faults leave the bound of every GPU case
@pytest.mark.parametrize("fault", S.FAULTS)
def test_planted_fault_leaves_the_bound_on_every_case(fault):
    for c in S.CASES:
        out, rx, rz = S.leaves_bound(c, fault)
        assert out, (S.case_id(c), fault, rx, rz)
        if fault in ("coupling_sign", "coupling_zprime", "stale_x"):
            assert rx == 0.0 and rz > 1.0, (S.case_id(c), fault, rx, rz)      # a fault of the z-step leaves x alone


def test_cases_cover_what_they_claim():
    shapes = lambda kind: {c.shape for c in S.CASES if c.kind == kind}
    assert shapes("spectral") == {(8, 8), (16, 8), (8, 64), (64, 128), (128, 32)}
    assert shapes("diag") == {(1, 9), (5, 7), (33, 70), (64, 136), (33, 72)}
    assert {c.prior for c in S.CASES} == {"tv", "aniso", "l1", "wavelet", "tgv"}
    assert sum(c.box is not None for c in S.CASES if c.kind == "spectral") == 1 and sum(c.box is not None for c in S.CASES if c.kind == "diag") == 1
    assert any(c.n_inner == 3 for c in S.CASES)
    for c in S.CASES:
        m = S.problem(c)
        if c.term == "mask" and c.kind == "diag":
            assert (m.m == 0).any()
        if c.term == "weights":
            assert (m.w == 0).any()
        if c.kind == "spectral" and c.term == "mask":
            assert (m.mask2 == 0).any()
        assert 0 < m.tau <= S.step_bound(m.rho, m.gamma)
