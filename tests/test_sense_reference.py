"""CPU-only: the reference of the multi-coil SENSE data term (tests/_sense_ref.py) held against itself -- the adjoint identity, the gradient against
central differences of the value, the single-coil case against the spectral term's reference, the Lipschitz bound against the power iteration, and
four planted faults that the per-pixel bound has to reject on every case."""
import numpy as np
import pytest

import _fourier_ref as F
import _sense_ref as S


@pytest.mark.parametrize("name", S.IDS)
@pytest.mark.parametrize("wkind", S.WEIGHTS)
def test_adjoint_identity_in_float64(name, wkind):
    c = S.case(name)
    A = S.SenseRef(S.maps(c.shape, c.n_coils), S.weight(c.shape, wkind))
    rng = np.random.default_rng(c.shape[1])
    x = rng.standard_normal(c.shape)
    k = rng.standard_normal((c.n_coils,) + c.shape) + 1j * rng.standard_normal((c.n_coils,) + c.shape)
    lhs, rhs = float(np.sum((A.forward(x) * np.conj(k)).real)), float(np.sum(x * A.adjoint(k)))      # the real inner product: x is real
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("name", S.IDS[:4])
def test_gradient_against_central_differences(name):
    c = S.case(name)
    m = S.problem(c.shape, c.n_coils, "weighted")
    t = S.term(m)
    x = m.x0[0].astype(np.float64)
    g = t.grad(x)
    rng = np.random.default_rng(3)
    for _ in range(5):      # f is quadratic: the central difference is exact up to rounding
        d = rng.standard_normal(c.shape)
        num = float(t.value(x + 0.5 * d) - t.value(x - 0.5 * d))
        assert abs(num - float(np.sum(g * d))) <= 1e-9 * max(abs(num), 1.0), (num, float(np.sum(g * d)))


@pytest.mark.parametrize("shape", [(8, 8), (16, 64)], ids=["8x8", "16x64"])
def test_one_coil_with_unit_map_is_the_spectral_term(shape):
    M = S.weight(shape, "weighted").astype(np.float64)
    x = F.operand(shape).astype(np.float64)
    rng = np.random.default_rng(1)
    b = 30 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    sense = S.SenseRef(np.ones((1,) + shape, dtype=np.complex128), M, b[None], 0.04)
    spec = F.SpectralRef(M.astype(np.complex128), b, 0.04)
    np.testing.assert_allclose(sense.grad(x), spec.grad(x), rtol=0, atol=1e-12 * np.max(np.abs(spec.grad(x))))
    np.testing.assert_allclose(sense.value(x), spec.value(x), rtol=1e-13)
    # max M^2 >= max_k (M_k^2 + M_-k^2) / 2, the spectral term's own bound for a real image
    assert sense.grad_lipschitz() >= spec.grad_lipschitz() * (1 - 1e-12)


@pytest.mark.parametrize("name", S.IDS)
@pytest.mark.parametrize("wkind", S.WEIGHTS)
def test_lipschitz_bound_holds_against_the_power_iteration(name, wkind):
    c = S.case(name)
    t = S.term(S.problem(c.shape, c.n_coils, wkind))
    lam = t.hessian_norm()
    print(f"L_f {name} {wkind}: bound {t.grad_lipschitz():.4e}, power iteration {lam:.4e}, ratio {t.grad_lipschitz() / lam:.2f}")
    assert t.grad_lipschitz() >= lam


@pytest.mark.parametrize("name", S.IDS)
def test_replay_is_single_precision_and_planted_faults_leave_the_bound(name):
    """m_once on the weighted M alone: with a binary M and masked data it is the same point (M^2 = M, M b = b up to the noise outside the mask, which
    M removes either way) -- the reason the weighted kind exists."""
    c = S.case(name)
    for wkind in S.WEIGHTS:
        m = S.problem(c.shape, c.n_coils, wkind)
        ref = S.grad_reference(c.shape, c.n_coils, wkind)
        assert ref.ref32.dtype == np.float32 and ref.ref64.dtype == np.float64
        assert 0 < ref.e32 < 1e-5, ref.e32
        for fault in S.FAULTS:
            if fault == "m_once" and wkind == "binary":
                continue
            err, _ = S.worst(S.term(m, np.float32, fault).grad(m.x0), ref.ref64)
            print(f"planted {fault} {name} {wkind}: err / bound {err / ref.bound:.1e}")
            assert err > 1e3 * ref.bound, (fault, wkind, err, ref.bound)
        good, _ = S.worst(ref.ref32, ref.ref64)
        assert good <= ref.bound


def test_step_references_are_built_in_both_precisions():
    for name in S.STEP_IDS:
        for st in S.step_reference(name):
            assert st.ref64.dtype == np.float64 and st.ref32.dtype == np.float32 and st.e32 > 0
            assert S.worst(st.ref32, st.ref64)[0] <= st.bound
