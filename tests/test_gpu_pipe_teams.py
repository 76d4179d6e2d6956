"""The two-team layout of the pipe kernel ('pipe2': 16 waves of 4 pixels per lane, each team on half the image width) against its
one-team layout ('pipe'): every pixel runs the same arithmetic on the same operands, only the place a neighbour value comes from
differs, so the chains' states must be equal bit for bit.  The energies and posterior moments are fp64 sums over pixels / chains formed
by other kernels with atomic adds, whose order varies from run to run: they are compared to 1e-12."""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")


def problem(shape, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros(shape)
    img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = 190.0
    img += np.linspace(0, 30, shape[1])[None, :]
    h = np.ones((5, 5)) / 25.0
    y = O.blur(img, h, (2, 2)) + rng.normal(0, 0.75, shape)
    return img, h, y, rng


def same(a, b, k):
    if k == "x":
        return np.array_equal(a, b)
    return np.allclose(a, b, rtol=1e-12, atol=0)


def run(la, variant, shape, C, nit, thin=1, noise="philox", x0=None):
    sigma, tau_reg = 0.75, 0.3
    img, h, y, rng = problem(shape, 5)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.TV(shape, sigma=tau_reg, niter=10)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C, tau=0.2 * sigma ** 2, gamma=sigma ** 2, seed=11, moments=True, thin=thin,
                          noise=noise, variant=variant)
    smp.set_state(img[None] + rng.normal(0, 10, (C,) + shape) if x0 is None else x0)
    smp.step(nit)
    out = {"x": smp.get_state().cpu().numpy()}
    f, g = smp.energies()
    out["f"], out["g"] = f.cpu().numpy(), g.cpu().numpy()
    s1, s2, cnt = smp.moments()
    out["s1"], out["s2"], out["cnt"] = s1.cpu().numpy(), s2.cpu().numpy(), np.asarray(cnt)
    name = smp.kernel_name
    smp.close()
    return out, name


@pytest.mark.parametrize("shape,C", [((512, 512), 3), ((37, 264), 4), ((41, 384), 2), ((23, 504), 2), ((1, 512), 2), ((6, 320), 5)])
def test_two_teams_equal_one_team(la, shape, C):
    one, n1 = run(la, "pipe", shape, C, 3)
    two, n2 = run(la, "pipe2", shape, C, 3)
    assert n1 == n2 == "myula_step_pipe_kernel"
    for k in one:
        assert same(one[k], two[k], k), (shape, k, float(np.max(np.abs(np.asarray(one[k], np.float64) - two[k]))))


def test_two_teams_through_the_sampler_with_thinning(la):
    # moments with thinning; no noise from a flat start, then with noise; auto picks the two-team layout for this configuration
    shape, C = (130, 448), 3
    for noise in ("none", "philox"):
        one, _ = run(la, "pipe", shape, C, 7, thin=3, noise=noise, x0=np.zeros(shape, np.float32))
        auto, _ = run(la, "auto", shape, C, 7, thin=3, noise=noise, x0=np.zeros(shape, np.float32))
        for k in one:
            assert same(one[k], auto[k], k), (noise, k)


@pytest.mark.parametrize("shape", [(40, 256), (40, 520), (40, 516)])
def test_two_teams_refuse_what_they_do_not_cover(la, shape):
    # below 264 / above 512 columns (or W % 8 != 0) the forced two-team variant refuses; auto still runs (one-team pipe or another kernel)
    sigma = 0.75
    img, h, y, _ = problem(shape, 1)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.TV(shape, sigma=0.3, niter=10)
    smp = la.MYULASampler(pf, pg, shape, n_chains=2, tau=0.2 * sigma ** 2, gamma=sigma ** 2, seed=1, variant="pipe2")
    smp.set_state(img)
    with pytest.raises(Exception):
        smp.step(1)
    smp.close()
