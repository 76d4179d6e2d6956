"""Uniform-box form of the pipe kernels' blur wave (lmc_step_pipe_uni.hip), per pixel: 5 x 5 box h = 1 / 25, one-team layout ('pipe') and, where it
covers the shape, the two-team layout ('pipe2'), against oracle.lmc_oracle.myula_step with injected noise -- the MAXIMUM ABSOLUTE error over pixels
after each of two iterations (the harness of tests/test_gpu_pipe_pairs.py).  Shapes, the smallest at which the shared-sum form can go wrong:

  (1, 512)   the vertical trees never fill
  (3, 264)   fewer rows than taps; smallest two-team width: right-aligned left team, seam
  (6, 264)   more rows than taps, same width
  (6, 256)   4 pixels per lane, every lane full
  (6, 132)   4 pixels per lane, empty tail lanes
  (7, 512)   both layouts at full width
  (6, 260)   not covered (rows not lane-aligned): runs the general form and must still pass

and one case of near-uniform taps at (6, 264): the first tap of the column factor of the (separable) box scaled by 1 + 1e-3 -- a whole row of h; a
single scaled entry of h is not separable and no pipe kernel takes it.  It must take the general form (the detection threshold is 1e-6 relative);
taken for a uniform box it would be wrong by 1e-3 / 5 of H x, some 0.04 on these states, against a bound of 5e-5.

Where both layouts cover a shape their states must be equal bit for bit: the sums are defined per pixel, whatever the lane layout.

Tolerance: per shape, twice the larger of the two iterations' errors this same file measures on the parent commit (5353a28), where the same inputs
take the general form.  Measured there (states are O(200), fp32 kernel against the fp64 oracle; iteration 1 / 2; one and two teams: the same figures):
  (1, 512) 1.689e-05 / 2.531e-05    (3, 264) 1.707e-05 / 2.399e-05    (6, 264) 1.767e-05 / 2.413e-05    (6, 256) 1.522e-05 / 2.210e-05
  (6, 132) 1.806e-05 / 2.185e-05    (7, 512) 1.660e-05 / 2.297e-05    (6, 260) 1.566e-05 / 2.129e-05    near-uniform (6, 264) 1.775e-05 / 2.338e-05
Measured with the uniform form (iteration 1 / 2; the same figures in both layouts):
  (1, 512) 1.689e-05 / 2.531e-05    (3, 264) 1.707e-05 / 2.592e-05    (6, 264) 1.767e-05 / 2.346e-05    (6, 256) 1.522e-05 / 2.210e-05
  (6, 132) 1.806e-05 / 2.185e-05    (7, 512) 1.660e-05 / 2.297e-05    (6, 260) and near-uniform: the parent's figures, the states are bit-identical
The uniform form exceeds the parent's own error on one shape, (3, 264), by 8 % (2.592e-05 against 2.399e-05); its states differ from the parent's by
at most 3.05e-05 (two units in the last place of a state of 200-odd) on every covered shape."""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

C, NIT = 2, 2
SHAPES = [(1, 512), (3, 264), (6, 264), (6, 256), (6, 132), (7, 512), (6, 260)]
NEAR = "near"           # the near-uniform case's key (shape (6, 264))
# largest per-pixel error of the parent commit over both layouts and both iterations (docstring)
PARENT_MAX_ERR = {(1, 512): 2.531e-05, (3, 264): 2.399e-05, (6, 264): 2.413e-05, (6, 256): 2.210e-05, (6, 132): 2.185e-05, (7, 512): 2.297e-05,
                  (6, 260): 2.129e-05, NEAR: 2.338e-05}


def teams_cover(shape):
    return 264 <= shape[1] <= 512 and shape[1] % 8 == 0


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")


_cache = {}


def reference(shape, near=False):
    """Problem and oracle states of a case, computed once and shared by the layouts (read only)."""
    key = (shape, near)
    if key not in _cache:
        sigma, tau_reg = 0.75, 0.3
        gamma, tau = sigma ** 2, 0.2 * sigma ** 2
        rng = np.random.default_rng(31)
        img = np.zeros(shape)
        img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = 190.0
        img += np.linspace(0, 30, shape[1])[None, :]
        h = np.ones((5, 5)) / 25
        if near:
            h[0, :] *= 1 + 1e-3
        y = O.blur(img, h, (2, 2)) + rng.normal(0, sigma, shape)
        x0 = img[None] + rng.normal(0, 10, (C,) + shape)
        noise = rng.standard_normal((NIT, C) + shape)
        op = {"kind": "tv", "sigma": tau_reg, "niter": 10, "t": gamma}
        xs, x = [], x0.copy()
        for it in range(NIT):
            x = O.myula_step(x, y, h, (2, 2), 1 / sigma ** 2, tau, gamma, op, noise[it])
            xs.append(x)
        for a in (h, y, x0, noise, *xs):
            a.setflags(write=False)
        _cache[key] = dict(h=h, y=y, x0=x0, noise=noise, xs=xs, sigma=sigma, tau_reg=tau_reg, gamma=gamma, tau=tau)
    return _cache[key]


def run(la, variant, shape, near=False):
    r = reference(shape, near)
    pf = la.L2(Op=la.Convolve2D(shape, r["h"], offset=(2, 2)), b=r["y"], sigma=1 / r["sigma"] ** 2)
    pg = la.TV(shape, sigma=r["tau_reg"], niter=10)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C, tau=r["tau"], gamma=r["gamma"], noise="injected", variant=variant)
    smp.set_state(r["x0"])
    states, errs = [], []
    for it in range(NIT):
        smp.step(1, noise=r["noise"][it:it + 1])
        got = smp.get_state().cpu().numpy()
        states.append(got)
        errs.append(float(np.max(np.abs(got.astype(np.float64) - r["xs"][it]))))
    name = smp.kernel_name
    smp.close()
    return states, errs, name


def check(la, shape, near, bound_key):
    layouts = ["pipe"] + (["pipe2"] if teams_cover(shape) else [])
    states, worst = {}, 0.0
    for v in layouts:
        states[v], errs, name = run(la, v, shape, near)
        assert name == "myula_step_pipe_kernel", (v, name)
        print(f"uni {bound_key} {v}: max abs error per iteration {errs[0]:.3e} {errs[1]:.3e}")
        worst = max(worst, *errs)
    assert worst <= 2.0 * PARENT_MAX_ERR[bound_key], (bound_key, worst, PARENT_MAX_ERR[bound_key])
    if len(layouts) == 2:
        for it in range(NIT):
            assert np.array_equal(states["pipe"][it], states["pipe2"][it]), (bound_key, it)


@pytest.mark.parametrize("shape", SHAPES)
def test_pipe_uni_per_pixel(la, shape):
    check(la, shape, False, shape)


def test_near_uniform_taps_take_the_general_form(la):
    check(la, (6, 264), True, NEAR)
