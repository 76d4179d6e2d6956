"""CPU-only: the harness of the Fourier-domain data term (tests/_fourier_ref.py) checked against itself -- the fold onto the half plane and the closed-form
prox against the definition on the full plane in float64, the periodic transfer function against the direct wrap-around sum (no FFT in that
reference), the dtype of the float32 replays, and planted faults: each must exceed the bound on every case where it applies."""
import numpy as np
import pytest

import _fourier_ref as F
import _pixel as X


def random_term(shape, seed):
    rng = np.random.default_rng(seed)
    cn = lambda: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return cn(), cn(), rng.normal(size=(2,) + shape)


@pytest.mark.parametrize("shape", F.FOLD_SHAPES, ids=[f"{h}x{w}" for h, w in F.FOLD_SHAPES])
def test_fold_prox_and_value_identities(shape):
    G, b, x = random_term(shape, 11)
    sigma, tau = 1.7, 0.6
    pf = F.SpectralRef(G, b, sigma)
    g_def = pf.grad(x)
    e_fold = np.max(np.abs(F.grad_folded(x, G, b, sigma) - g_def))
    p = pf.prox(x, tau)
    e_prox = np.max(np.abs(p - x + tau * pf.grad(p)))
    e_val = np.max(np.abs(F.value_half(x, G, b, sigma) - pf.value(x)) / pf.value(x))
    print(f"{shape}: fold {e_fold:.2e}, prox optimality {e_prox:.2e}, value rel {e_val:.2e}")
    assert e_fold <= 5e-14 and e_prox <= 5e-14 and e_val <= 1e-14
    # finite differences of the value against the gradient, along a random direction
    d = np.random.default_rng(3).normal(size=x.shape)
    h = 1e-5
    fd = (pf.value(x + h * d) - pf.value(x - h * d)) / (2 * h)
    an = np.sum(g_def * d, axis=(-2, -1))
    assert np.allclose(fd, an, rtol=1e-7), (fd, an)
    assert pf.grad_lipschitz() == pytest.approx(sigma * np.max(0.5 * (np.abs(G) ** 2 + np.abs(F.minus_k(G)) ** 2)))


def test_tables_zero_the_second_residual_in_the_self_conjugate_columns():
    G, b, _ = random_term((16, 64), 5)
    t = F.tables(G, b)
    assert t.shape == (11, 16, 33)
    for j in (0, 32):
        assert not t[7:, :, j].any() and t[3:7, :, j].all()
    assert t[7:, :, 1:32].all()


@pytest.mark.parametrize("name", F.CONV_IDS)
def test_periodic_transfer_matches_the_direct_sum(name):
    c = F.CONV_CASES[F.CONV_IDS.index(name)]
    x = F.operand(c.shape)[0].astype(np.float64)
    G = F.periodic_gain(c.shape, c.h, c.offset)
    for adjoint in (False, True):
        via = np.fft.ifft2((np.conj(G) if adjoint else G) * np.fft.fft2(x)).real
        direct = F.periodic_direct(x, c.h, c.offset, adjoint)
        e = np.max(np.abs(via - direct)) / np.max(np.abs(direct))
        assert e <= 3e-15, (name, adjoint, e)
    r = np.random.default_rng(1).normal(size=c.shape)
    assert np.sum(F.periodic_direct(x, c.h, c.offset) * r) == pytest.approx(np.sum(x * F.periodic_direct(r, c.h, c.offset, True)), rel=1e-12)


@pytest.mark.parametrize("shape", F.SHAPES, ids=F.SHAPE_IDS)
def test_replays_are_single_precision_and_faults_exceed_the_bound(shape):
    ref = F.rfft2_reference(shape)
    assert ref.ref32.dtype == np.float32 and ref.e32 > 0 and ref.bound >= 3 * ref.e32
    x = ref.x.astype(np.float64)
    for fault in F.TRANSFORM_FAULTS:
        if fault is F.fault_transposed and shape[0] == shape[1]:
            continue
        err, _ = F.worst(F.ri(fault(x)), ref.ref64)
        print(f"{shape} {fault.__name__}: err {err:.3e}, bound {ref.bound:.3e}")
        assert err > ref.bound, (fault.__name__, err, ref.bound)
    rt = F.roundtrip_reference(shape)
    ir = F.irfft2_reference(shape)
    assert rt.e32 > 0 and ir.e32 > 0
    # the conjugate direction on the way back, and 1 / N
    c = ir.x.astype(np.complex128)
    for bad in (np.fft.irfft2(np.conj(c), s=shape, norm="ortho"), np.fft.irfft2(c, s=shape, norm="backward")):
        assert F.worst(bad, ir.ref64)[0] > ir.bound


@pytest.mark.parametrize("name", [n for n in F.STEP_IDS if n.startswith("grad") or n in ("wmask-l1", "transfer-tvpos")])
def test_fold_and_mask_faults_exceed_the_step_bound(name):
    m = F.step_problem(name)
    st = F.step_reference(name)[0]
    x = st.start.astype(np.float64)
    good = F.grad_folded(x, m.G, m.b, m.sigma_f)
    scale = 1.0 if name.startswith("grad") else m.tau      # a step carries the gradient times tau
    _, gbound = X.bound_of(F.SpectralRef(m.G, m.b, m.sigma_f).grad(x), F.SpectralRef(m.G, m.b, m.sigma_f, np.float32).grad(st.start))
    assert np.max(np.abs(good - F.SpectralRef(m.G, m.b, m.sigma_f).grad(x))) <= gbound
    at_k = F.grad_folded(x, m.G, m.b, m.sigma_f, fold_fn=F.fold_at_k)
    e = np.max(np.abs(at_k - good)) * scale
    print(f"{name}: fold at k {e:.3e}, bound {st.bound:.3e}")
    assert e > st.bound
    if m.mask is not None:
        Gs = m.G * 0 + F.mask_shifted(m.mask) * (m.G / np.where(m.mask > 0, m.mask, 1.0) if m.transfer is not None or m.weights is not None else 1.0)
        e = np.max(np.abs(F.grad_folded(x, Gs, m.b, m.sigma_f) - good)) * scale
        print(f"{name}: shifted mask {e:.3e}, bound {st.bound:.3e}")
        assert e > st.bound


def test_step_cases_cover_the_issue():
    assert F.STEP_IDS == ["mask-tv10-pipe", "mask-tv10-split", "wmask-l1", "transfer-tvpos", "periodic15-aniso", "periodic-wavelet", "grad-8x8", "grad-128x256"]
    for name in F.STEP_IDS:
        m = F.step_problem(name)
        assert m.tau * F.SpectralRef(m.G, m.b, m.sigma_f).grad_lipschitz() < 1.0
        if m.mask is not None:
            assert m.mask[:2, :2].all() and m.mask[-2:, -2:].all() and 0.2 < m.mask.mean()
            assert m.mask.size < 1024 or m.mask.mean() < 0.4          # (8 x 8: the 4 x 4 centre is a quarter of the plane)
            assert not np.allclose(m.b, np.conj(F.minus_k(m.b)))          # the data are not Hermitian
