"""CPU only: the harness of tests/test_gpu_huber.py checked on itself.  The reference of tests/_huber_ref.py against a central finite difference of its
own value and for continuity at |r| = delta; the recipe's figures; and the planted faults -- the wrong kernels a Huber data term could be -- which the
comparisons must reject at the GPU tolerances (rel-L2 1e-5, the per-pixel bound of tests/_pixel.py, energies rtol 5e-5) on every shape the GPU file uses."""
import functools

import numpy as np
import pytest

import _huber_ref as R
import _pixel as PX

SHAPES = [(20, 33), (24, 136), (24, 264), (40, 128)]
OPS = ["blur5", "identity"]


@functools.lru_cache(maxsize=None)
def case(shape, data):
    op = R.Op("blur", *R.box_kernel(5)) if data == "blur5" else R.Op("identity")
    _, op, y, d, x0 = R.recipe(shape, op=op)
    return op, y, d, x0


@pytest.mark.parametrize("data", OPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_recipe_meets_the_conditions(shape, data):
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, R.SIGMA_F)
    clipped, zero, inf, d_grad, d_step, d_f = R.assert_discriminates(ref, x0, R.STEP_TOL)
    print(f"{data} {shape}: clipped {clipped:.2f}, delta=0 {zero:.2f}, delta=inf {inf:.2f}, wrong gradients {d_grad}, wrong step {d_step:.2e}, L2 value {d_f:.2f}")
    assert (np.asarray(ref.plain_value(x0)) > 3 * np.asarray(ref(x0))).all()
    for a in (y, x0, d[np.isfinite(d)]):
        assert np.array_equal(a, R.f32(a)), "the inputs are float32 numbers"


@pytest.mark.parametrize("data", OPS)
def test_gradient_is_the_finite_difference_of_the_value(data):
    shape = (20, 33)
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, 1.3 * R.SIGMA_F)
    x = x0[0]
    g = ref.grad(x)
    rng = np.random.default_rng(1)
    eps = 1e-4
    for _ in range(8):      # directional derivatives: h is C^1 and piecewise quadratic, so the central difference errs by O(eps) only at the kinks it straddles
        v = rng.standard_normal(shape)
        fd = (ref(x + eps * v) - ref(x - eps * v)) / (2 * eps)
        assert abs(fd - np.sum(g * v)) <= 1e-6 * np.linalg.norm(g) * np.linalg.norm(v), (fd, np.sum(g * v))


def test_value_and_derivative_are_continuous_at_the_threshold():
    d = np.array([0.0, 0.5, 3.0, 12.0])
    for s in (-1.0, 1.0):
        for eps in (1e-9, -1e-9):      # just outside and just inside the threshold: both branches give delta^2 / 2 and +-delta there
            r = s * (d + eps)
            assert np.allclose(R.huber(r, d), d * d / 2, rtol=0, atol=1e-7 * (1 + d))
            assert np.allclose(R.psi(r, d), s * d, rtol=0, atol=2e-9)
    r = np.array([-7.0, 0.0, 2.5])
    assert np.array_equal(R.huber(r, np.full(3, np.inf)), r * r / 2) and np.array_equal(R.psi(r, np.full(3, np.inf)), r)
    assert np.array_equal(R.huber(r, np.zeros(3)), np.zeros(3)) and np.array_equal(np.abs(R.psi(r, np.zeros(3))), np.zeros(3))
    assert R.huber(np.float32(20.0), np.float32(4.0)).dtype == np.float32 and R.huber(np.float32(20.0), np.float32(4.0)) == 4.0 * (20.0 - 2.0)


def pixel_bound(op, y, d, x0, sigma):
    """(ref64, bound) of the gradient: max(3 e32, 2 ulp32(max |ref64|)), e32 from the reference's own float32 replay."""
    ref64 = R.HuberRef(op, y, d, sigma).grad(x0)
    ref32 = R.HuberRef(op, y, d, sigma, dtype=np.float32).grad(x0.astype(np.float32))
    assert ref32.dtype == np.float32
    return ref64, PX.bound_of(ref64, ref32)[1]


@pytest.mark.parametrize("data", OPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_planted_gradient_faults_are_rejected(shape, data):
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, R.SIGMA_F)
    want, bound = pixel_bound(op, y, d, x0, R.SIGMA_F)
    assert R.rel(ref.grad(x0), want) == 0.0
    faults = R.wrong_gradients(ref)
    assert set(faults) >= {"delta ignored", "clamp of Op x", "planes swapped", "times delta"} and ("clamp after the adjoint" in faults) == (data == "blur5")
    for name, fn in faults.items():
        got = fn(x0)
        e = R.distance(got, want)
        worst = float(np.max(np.abs(got - want))) if np.isfinite(got).all() else np.inf
        print(f"{data} {shape} {name}: rel {e:.3e}, worst pixel {worst:.3e} against the bound {bound:.3e}")
        assert not e < R.STEP_TOL, (name, e)
        assert not worst <= bound, (name, worst, bound)
    # the float32 replay itself passes both: the bound is no tighter than the device's number format
    r32 = R.HuberRef(op, y, d, R.SIGMA_F, dtype=np.float32).grad(x0.astype(np.float32)).astype(np.float64)
    assert R.rel(r32, want) < R.STEP_TOL and np.max(np.abs(r32 - want)) <= bound


@pytest.mark.parametrize("data", OPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_planted_value_faults_are_rejected(shape, data):
    op, y, d, x0 = case(shape, data)
    ref = R.HuberRef(op, y, d, R.SIGMA_F)
    want = np.asarray(ref(x0))
    for name, fn in (("L2 value", ref.plain_value), ("linear branch without -delta^2/2", ref.value_without_offset)):
        got = np.asarray(fn(x0))
        e = np.max(np.abs(got - want) / np.abs(want))
        print(f"{data} {shape} {name}: relative {e:.3e}")
        assert np.min(np.abs(got - want) / np.abs(want)) > R.ENERGY_RTOL, (name, e)
    with np.errstate(invalid="ignore"):
        swapped = np.asarray(R.HuberRef(op, d, y, R.SIGMA_F)(x0))     # the planes swapped: y = +inf at a tenth of the pixels
    assert not (np.abs(swapped - want) / np.abs(want) < R.ENERGY_RTOL).any()
    v32 = np.asarray(R.HuberRef(op, y, d, R.SIGMA_F, dtype=np.float32)(x0.astype(np.float32)), dtype=np.float64)
    assert np.max(np.abs(v32 - want) / np.abs(want)) < R.ENERGY_RTOL
