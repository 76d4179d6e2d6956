"""Pixel pairing of the pipe kernels, per pixel: the smallest shapes at which the neighbour logic of a lane's pixel pairs can go wrong,
one-team layout ('pipe') and, where it covers the shape, the two-team layout ('pipe2'), against oracle.lmc_oracle.myula_step with injected
noise -- the MAXIMUM ABSOLUTE error over pixels after each of two iterations (a norm would average a single wrong column away).

  (6, 132)            4 pixels per lane, empty tail lanes
  (6, 256)            4 pixels per lane, every lane full
  (6, 260)            8 pixels per lane, last column in mid-lane, rows not lane-aligned (pixel-by-pixel instantiation)
  (6, 264)            smallest two-team width: right-aligned left team, seam
  (1, 512), (6, 512)  full width, both layouts
  (6, 520)            two column strips

Tolerance: twice the largest per-pixel error of the commit before the pairing changed (2175914), measured with this file; the kernels are
bit-identical to that commit's, the factor 2 only guards against another reduction order in the oracle's BLAS.  Measured (states are
O(200), fp32 kernel against the fp64 oracle; iteration 1 / 2):
  (6, 132) 1.602e-05 / 2.368e-05    (6, 256) 1.563e-05 / 2.403e-05    (6, 260) 1.704e-05 / 2.208e-05    (6, 264) 1.610e-05 / 2.406e-05
  (1, 512) 1.458e-05 / 2.028e-05    (6, 512) 1.639e-05 / 2.397e-05    (6, 520) 1.658e-05 / 2.487e-05    (one and two teams: the same figures)
Where both layouts cover a shape their states must be equal bit for bit: they pair different pixels ((i, i + 4) and (i, i + 2)), so a
pairing mistake cannot cancel."""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

C, NIT = 2, 2
SHAPES = [(6, 132), (6, 256), (6, 260), (6, 264), (1, 512), (6, 512), (6, 520)]
# largest per-pixel error of the parent commit over both layouts and both iterations (docstring)
PARENT_MAX_ERR = {(6, 132): 2.368e-05, (6, 256): 2.403e-05, (6, 260): 2.208e-05, (6, 264): 2.406e-05, (1, 512): 2.028e-05, (6, 512): 2.397e-05,
                  (6, 520): 2.487e-05}


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


def reference(shape):
    """Problem and oracle states of a shape, computed once and shared by the layouts (read only)."""
    if shape not in _cache:
        sigma, tau_reg = 0.75, 0.3
        gamma, tau = sigma ** 2, 0.2 * sigma ** 2
        rng = np.random.default_rng(29)
        img = np.zeros(shape)
        img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = 190.0
        img += np.linspace(0, 30, shape[1])[None, :]
        h = np.outer([1, 2, 3, 2, 1], [1, 3, 4, 2, 1]).astype(np.float64)      # asymmetric columns: a mirrored tap or neighbour shows
        h /= h.sum()
        y = O.blur(img, h, (2, 2)) + rng.normal(0, sigma, shape)
        x0 = img[None] + rng.normal(0, 10, (C,) + shape)
        noise = rng.standard_normal((NIT, C) + shape)
        op = {"kind": "tv", "sigma": tau_reg, "niter": 10, "t": gamma}
        xs, x = [], x0.copy()
        for it in range(NIT):
            x = O.myula_step(x, y, h, (2, 2), 1 / sigma ** 2, tau, gamma, op, noise[it])
            xs.append(x)
        for a in (y, x0, noise, *xs):
            a.setflags(write=False)
        _cache[shape] = dict(h=h, y=y, x0=x0, noise=noise, xs=xs, sigma=sigma, tau_reg=tau_reg, gamma=gamma, tau=tau)
    return _cache[shape]


def run(la, variant, shape):
    r = reference(shape)
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


@pytest.mark.parametrize("shape", SHAPES)
def test_pipe_pairs_per_pixel(la, shape):
    layouts = ["pipe"] + (["pipe2"] if teams_cover(shape) else [])
    states, worst = {}, 0.0
    for v in layouts:
        states[v], errs, name = run(la, v, shape)
        assert name == "myula_step_pipe_kernel", (v, name)
        print(f"pairs {shape} {v}: max abs error per iteration {errs[0]:.3e} {errs[1]:.3e}")
        worst = max(worst, *errs)
    assert worst <= 2.0 * PARENT_MAX_ERR[shape], (shape, worst, PARENT_MAX_ERR[shape])
    if len(layouts) == 2:
        for it in range(NIT):
            assert np.array_equal(states["pipe"][it], states["pipe2"][it]), (shape, it)
