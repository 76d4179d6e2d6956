"""A sampler handle works in buffers of its own: its trajectory does not depend on what else runs in the process.

For four configurations whose work buffers come from the host code's one sizing-and-binding function (a large PSF with its energies, the spectral
term with the wavelet prior, the 1-D inner prox of the anisotropic ME-TV term under ULPDA, the pass-by-pass early exit of the ME-TV inner prox on a
narrow image), handle A (3 chains) and handle B (5 chains, another seed) are first run alone, then interleaved in one process with each other and with
stateless lmc_fused_eval / lmc_energies calls of the same problem on 7 images, which grow the device's workspace between A's steps.  The interleaved
states must equal the solo ones byte for byte; the energies to rtol 1e-12, the project's allowance for the atomically summed float64 energies
(scripts/compare_dumps.py).  One stream, no threads: a guard of the sizing and binding, not a race detector."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (16, 16)      # the spectral term takes powers of two >= 8, db2 with 2 levels multiples of 4
TAU, GAMMA = 0.1, 0.5
ENERGY_RTOL = 1e-12


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import lmc_atomi_amd as la
    return la


def observation(seed=0):
    rng = np.random.default_rng(seed)
    img = np.zeros(SHAPE)
    img[4:11, 3:12] = 4.0
    return img, rng


def psf_tv(la, n_chains, seed):
    img, rng = observation()
    h = rng.uniform(0.2, 1.0, (9, 9))      # no outer product: the general form
    h /= h.sum()
    y = (img + rng.normal(0, 0.3, SHAPE)).astype(np.float32)
    pf = la.L2(Op=la.PSF(SHAPE, h.astype(np.float32), offset=(4, 4), separable=False), b=y, sigma=2.0)
    return la.MYULASampler(pf, la.TV(SHAPE, sigma=0.3, niter=10), SHAPE, n_chains=n_chains, tau=TAU, gamma=GAMMA, seed=seed)


def spectral_wavelet(la, n_chains, seed):
    img, rng = observation()
    mask = (rng.uniform(size=SHAPE) < 0.6).astype(np.float64)
    mask[0, 0] = 1.0
    y = mask * np.fft.fft2(img, norm="ortho") + mask * (rng.normal(0, 0.1, SHAPE) + 1j * rng.normal(0, 0.1, SHAPE))
    pf = la.L2(Op=la.FourierSampling(SHAPE, mask), b=y, sigma=2.0)
    return la.MYULASampler(pf, la.WaveletL1(SHAPE, sigma=0.3, levels=2, wavelet="db2"), SHAPE, n_chains=n_chains, tau=TAU, gamma=GAMMA, seed=seed)


def ulpda_me_aniso(la, n_chains, seed):
    img, rng = observation()
    y = (img + rng.normal(0, 0.3, SHAPE)).astype(np.float32)
    pf = la.L2_ncvx_tv(dims=SHAPE, Op=la.Identity(SHAPE[0] * SHAPE[1]), b=y.ravel(), sigma=2.0, lamda=0.3, gamma=2.0, isotropic=False, niter=6, rtol=0.0)
    return la.ULPDASampler(pf, la.L21(sigma=0.3), la.Gradient(SHAPE), SHAPE, n_chains=n_chains, tau=0.2, mu=0.5, seed=seed)


def me_pass_by_pass(la, n_chains, seed):
    img, rng = observation()
    y = (img + rng.normal(0, 0.3, SHAPE)).astype(np.float32)
    h = np.ones((3, 3), np.float32) / 9.0
    pf = la.L2_ncvx_tv(dims=SHAPE, Op=la.Convolve2D(SHAPE, h, offset=(1, 1)), b=y.ravel(), sigma=2.0, lamda=0.3, gamma=2.0, isotropic=True, niter=12,
                       rtol=1e-4)      # W = 16: the full-width pipeline does not cover it, the early exit runs pass by pass
    return la.MYULASampler(pf, la.TV(SHAPE, sigma=0.3, niter=10), SHAPE, n_chains=n_chains, tau=TAU, gamma=GAMMA, seed=seed)


CONFIGS = {"psf-tv-energies": psf_tv, "spectral-wavelet": spectral_wavelet, "ulpda-me-tv-aniso": ulpda_me_aniso, "me-tv-pass-by-pass": me_pass_by_pass}
A = dict(n_chains=3, seed=11)
B = dict(n_chains=5, seed=23)


def snapshot(smp):
    f, g = smp.energies()
    return smp.get_state().cpu().numpy().copy(), f.cpu().numpy().copy(), g.cpu().numpy().copy()


def solo(la, make, who, n_steps):
    smp = make(la, **who)
    try:
        smp.step(n_steps)
        return snapshot(smp)
    finally:
        smp.close()


def same(what, got, want):
    x, f, g = got
    x0, f0, g0 = want
    assert np.isfinite(x0).all() and np.any(x0 != 0.0), what
    assert x.tobytes() == x0.tobytes(), (what, float(np.max(np.abs(x.astype(np.float64) - x0))))
    for name, e, e0 in (("f", f, f0), ("g", g, g0)):
        worst = float(np.max(np.abs(e - e0) / np.maximum(np.abs(e0), 1e-300)))
        print(f"{what}: energy {name} worst relative difference {worst:.3e} (allowed {ENERGY_RTOL:.0e})")
        np.testing.assert_allclose(e, e0, rtol=ENERGY_RTOL, atol=0.0, err_msg=f"{what} {name}")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_interleaved_handles_and_stateless_calls_leave_each_handle_alone(la, name):
    make = CONFIGS[name]
    want_a = solo(la, make, A, 3)
    want_b = solo(la, make, B, 2)
    a, b = make(la, **A), make(la, **B)
    try:
        a.step(1)
        b.step(1)
        # the same problem on 7 images through the stateless calls: the device's workspace grows past both handles
        x7 = np.random.default_rng(5).normal(2.0, 1.0, (7,) + SHAPE).astype(np.float32)
        out = a._problem.eval(x7, 0.8, TAU, 0.2, GAMMA)
        f7, g7 = a._problem.energies(x7)
        assert np.isfinite(np.asarray(out)).all() and np.isfinite(f7.cpu().numpy()).all() and np.isfinite(g7.cpu().numpy()).all()
        a.step(2)
        b.step(1)
        same(f"{name} handle A", snapshot(a), want_a)
        same(f"{name} handle B", snapshot(b), want_b)
    finally:
        a.close()
        b.close()
