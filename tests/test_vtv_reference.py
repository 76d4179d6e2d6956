"""CPU only: holds tests/_vtv_ref.py -- the numpy restatement of the vectorial TV prior that tests/test_gpu_vtv.py measures the kernels against -- to
the properties of the definition (include/lmc_atomi.h, LMC_PRIOR_VTV), and plants the faults a coupled prox can have: each must exceed the bound of every
case of the GPU list, or the bound could not tell the coupled prox from a wrong one."""
import numpy as np
import pytest

from oracle import lmc_oracle as O
import _vtv_ref as V

SMALL = [(5, 7), (16, 24), (33, 70)]


def _x64(shape, nch):
    return V.images(shape, nch).astype(np.float64)


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_channel_is_the_isotropic_tv_prox_bit_for_bit(shape, dtype):
    x = V.images(shape, 1).astype(dtype)
    for t, K in [(0.75, 1), (2.5, 10), (40.0, 23)]:
        got = V.vtv_prox(x, t, K)
        ref = O.tv_prox_fgp(x[:, 0], t, K)
        assert got.dtype == ref.dtype == dtype
        assert np.array_equal(got[:, 0], ref), (shape, t, K)
    assert np.allclose(V.vtv_value(x.astype(np.float64)), [float(O.tv_value(im[0])) for im in x.astype(np.float64)], rtol=1e-13, atol=0)


@pytest.mark.parametrize("nch", [2, 3])
def test_an_infinite_box_is_no_box_and_a_finite_one_is_not_a_clip_afterwards(nch):
    x = _x64((16, 24), nch)
    free = V.vtv_prox(x, 2.5, 10)
    assert np.array_equal(V.vtv_prox(x, 2.5, 10, bounds=(-np.inf, np.inf)), free)
    lo, hi = 60.0, 170.0
    boxed = V.vtv_prox(x, 2.5, 10, bounds=(lo, hi))
    assert boxed.min() >= lo and boxed.max() <= hi
    gap = np.max(np.abs(boxed - np.clip(free, lo, hi)))
    print(f"constrained prox vs clip afterwards: {gap:.3f} grey levels")
    assert gap > 0.1


@pytest.mark.parametrize("nch", [2, 3, 4])
def test_the_prox_commutes_with_an_orthogonal_mixing_of_the_channels(nch):
    """VTV sees the channels through sum_ch of squares alone, so Q x has the prox Q prox(x) for every orthogonal Q -- every truncated iterate too."""
    rng = np.random.default_rng(nch)
    Q, _ = np.linalg.qr(rng.normal(size=(nch, nch)))
    x = _x64((16, 24), nch)
    mix = lambda a: np.einsum("ab,nbij->naij", Q, a)
    err = np.max(np.abs(V.vtv_prox(mix(x), 2.5, 10) - mix(V.vtv_prox(x, 2.5, 10))))
    print(f"nch {nch}: |prox(Qx) - Q prox(x)| = {err:.2e}")
    assert err < 1e-11
    assert np.allclose(V.vtv_value(mix(x)), V.vtv_value(x), rtol=1e-13)


def test_the_iterates_descend_to_the_minimiser_of_the_primal_objective():
    x = _x64((16, 24), 3)[:1]
    t = 2.5
    obj = lambda u: 0.5 * np.sum((u - x) ** 2) + t * float(V.vtv_value(u)[0])
    o10, o50, o400 = (obj(V.vtv_prox(x, t, K)) for K in (10, 50, 400))
    print(f"objective at K = 10, 50, 400: {o10:.6f} {o50:.6f} {o400:.6f}")
    assert o50 <= o10 and o400 <= o50
    u = V.vtv_prox(x, t, 3000)
    rng = np.random.default_rng(0)
    for _ in range(20):
        assert obj(u) < obj(u + 1e-3 * rng.normal(size=u.shape))


FAULTS = ["independent", "drop_last", "max", "columns_uncoupled"]
MULTI = [(s, n) for s in V.SHAPES for n in V.CHANNELS if n >= 2]


@pytest.mark.parametrize("shape,nch", MULTI, ids=[f"{s[0]}x{s[1]}-{n}ch" for s, n in MULTI])
def test_planted_faults_exceed_the_bound_of_every_case(shape, nch):
    x = V.images(shape, nch).astype(np.float64)
    smallest = np.inf
    for t in V.PROX_PARAMS:
        for K in V.ITERS:
            ref64, e32, bound = V.prox_reference(shape, nch, t, K)
            if (t, K) == (40.0, 1):
                # one dual step of 1 / (8 * 40) of these gradients stays inside the unit ball channel by channel, and jointly everywhere but at the corner
                # pixels of the block, where a row and a column jump of every channel meet (2 (190^2 + 150^2) / 320^2 = 1.14): the reference itself projects
                # next to nothing, so the forms of the projection cannot be told apart and the case is no fault case
                _, (r, s) = V.vtv_prox(x, t, K, return_dual=True)
                assert np.max(r * r + s * s) <= 1.0
                assert np.max(np.sum(np.sum(r * r + s * s, axis=-3) > 1.0, axis=(-2, -1))) <= 4
                continue
            for fault in FAULTS:
                dev = float(np.max(np.abs(V.vtv_prox(x, t, K, planted=fault) - ref64)))
                smallest = min(smallest, dev / bound)
                assert dev > bound, (fault, shape, nch, t, K, dev, bound)
    print(f"{shape} x {nch} channels: smallest planted deviation / bound = {smallest:.3g}")


def test_the_coupled_prox_is_not_the_channels_run_alone():
    for shape, nch, t in [((16, 24), 2, 0.75), ((33, 70), 3, 2.5), ((97, 261), 4, 40.0)]:
        x = _x64(shape, nch)
        alone = np.stack([O.tv_prox_fgp(x[:, ch], t, 10) for ch in range(nch)], axis=1)
        gap = np.max(np.abs(V.vtv_prox(x, t, 10) - alone))
        print(f"{shape} x {nch} channels, t = {t}: coupled vs independent {gap:.2f} grey levels")
        assert gap > 0.5


def test_the_step_is_the_formula():
    rng = np.random.default_rng(5)
    nch, C, shape = 3, 2, (16, 24)
    x = rng.normal(100, 20, (nch, C) + shape)
    y = rng.normal(100, 20, (nch,) + shape)
    xi = rng.standard_normal(x.shape)
    h = np.ones((5, 5)) / 25.0
    tau, gamma, ts = 0.1, 0.5, 0.4
    got = V.myula_step(x, y, h, (2, 2), None, 2.0, tau, gamma, ts, 10, xi)
    px = np.moveaxis(V.vtv_prox(np.moveaxis(x, 0, 1), ts, 10), 1, 0)
    g = 2.0 * O.blur_adjoint(O.blur(x, h, (2, 2)) - y[:, None], h, (2, 2))
    assert np.allclose(got, (1 - tau / gamma) * x - tau * g + (tau / gamma) * px + np.sqrt(2 * tau) * xi, rtol=0, atol=1e-12)
