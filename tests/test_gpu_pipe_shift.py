"""Wave shifts folded into the differences that use them (sub_left_pair, right_pair_sub, pipe_cdown; lmc_step_pipe_kernel.h), per pixel: a wrong
neighbour at the end of a lane, at the team seam or in the first / last row must show at O(1), not at rounding level.  The inputs are therefore ZERO
images with single bright pixels -- in the state (200 in chain 0, 120 in chain 1) and in the observation (150) -- at

  columns 0, 3, 4, W/2 - 1, W/2, W - 1      (a lane's first and last pixel at 4 pixels per lane, both sides of the seam, the image's edges)
  rows    0, H - 1

and every case runs 1 and 2 MYULA steps (TV, K = 10) with the noise off and with the device's Philox noise, against oracle.lmc_oracle.myula_step in
float64 (the Philox field from oracle.philox_normals).  Shapes, the smallest of tests/test_gpu_pipe_pairs.py:

  (3, 264) (6, 264) (24, 264)   two teams, narrowest width; fewer rows than the pipeline is deep, and more
  (6, 512)                      two teams, full width
  (6, 256)                      one team, 4 pixels per lane, every lane full
  (6, 264) 'pipe'               one team, 8 pixels per lane, the layout chosen through set_step_variant

with the uniform 5 x 5 box (the uniform-box kernels) and with the asymmetric taps of test_gpu_pipe_pairs.py (the general kernels).  Where both layouts
cover a shape (W >= 264) they run both and must agree bit for bit.

Bound: the maximum absolute error per pixel is at most TWICE the figure the parent build (df46979) gives on the same inputs (the margin of
tests/test_gpu_pipe_fold.py: each pixel gets the same IEEE operations on the same operands, the factor covers another reduction order in the checker's
BLAS).  PARENT below is that measurement, max over the layouts, after step 1 and step 2; profiles/r09_shift_parity.txt holds both builds' figures."""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

C, NIT, SEED = 2, 2, 11
AMP_X, AMP_Y = (200.0, 120.0), 150.0
# (shape, how the layout is chosen): 'both' = variant 'pipe' and 'pipe2' on the sampler; 'pipe' = variant 'pipe' alone; 'global-pipe' = set_step_variant('pipe')
CASES = [((3, 264), "both"), ((6, 264), "both"), ((24, 264), "both"), ((6, 512), "both"), ((6, 256), "pipe"), ((6, 264), "global-pipe")]
NOISES = ["none", "philox"]
BLURS = ["box", "asym"]
# parent build: max abs error per pixel after step 1 and after step 2 (max over the layouts run), measured with this file
PARENT = {
    ((3, 264), 'both', 'none', 'box'): (6.903e-06, 1.608e-05),
    ((6, 264), 'both', 'none', 'box'): (7.446e-06, 1.517e-05),
    ((24, 264), 'both', 'none', 'box'): (7.447e-06, 1.941e-05),
    ((6, 512), 'both', 'none', 'box'): (7.446e-06, 1.517e-05),
    ((6, 256), 'pipe', 'none', 'box'): (7.446e-06, 1.517e-05),
    ((6, 264), 'global-pipe', 'none', 'box'): (7.446e-06, 1.517e-05),
    ((3, 264), 'both', 'philox', 'box'): (7.690e-06, 1.175e-05),
    ((6, 264), 'both', 'philox', 'box'): (8.911e-06, 1.011e-05),
    ((24, 264), 'both', 'philox', 'box'): (8.910e-06, 1.277e-05),
    ((6, 512), 'both', 'philox', 'box'): (8.911e-06, 1.240e-05),
    ((6, 256), 'pipe', 'philox', 'box'): (8.911e-06, 1.018e-05),
    ((6, 264), 'global-pipe', 'philox', 'box'): (8.911e-06, 1.011e-05),
    ((3, 264), 'both', 'none', 'asym'): (8.027e-06, 1.527e-05),
    ((6, 264), 'both', 'none', 'asym'): (5.978e-06, 1.521e-05),
    ((24, 264), 'both', 'none', 'asym'): (5.978e-06, 8.094e-06),
    ((6, 512), 'both', 'none', 'asym'): (5.978e-06, 1.521e-05),
    ((6, 256), 'pipe', 'none', 'asym'): (5.978e-06, 1.521e-05),
    ((6, 264), 'global-pipe', 'none', 'asym'): (5.978e-06, 1.521e-05),
    ((3, 264), 'both', 'philox', 'asym'): (9.013e-06, 1.545e-05),
    ((6, 264), 'both', 'philox', 'asym'): (8.894e-06, 9.281e-06),
    ((24, 264), 'both', 'philox', 'asym'): (8.019e-06, 1.563e-05),
    ((6, 512), 'both', 'philox', 'asym'): (8.019e-06, 1.607e-05),
    ((6, 256), 'pipe', 'philox', 'asym'): (8.019e-06, 1.676e-05),
    ((6, 264), 'global-pipe', 'philox', 'asym'): (8.894e-06, 9.281e-06),
}


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")


def spikes(shape, amp):
    H, W = shape
    a = np.zeros(shape)
    for r in (0, H - 1):
        for c in (0, 3, 4, W // 2 - 1, W // 2, W - 1):
            a[r, c] = amp
    return a


_cache = {}


def reference(shape, noise, blur):
    """Problem and checker states of a case, computed once and shared by the layouts (read only)."""
    key = (shape, noise, blur)
    if key not in _cache:
        sigma, tau_reg = 0.75, 0.3
        gamma, tau = sigma ** 2, 0.2 * sigma ** 2
        h = np.ones((5, 5)) / 25 if blur == "box" else np.outer([1, 2, 3, 2, 1], [1, 3, 4, 2, 1]).astype(np.float64)
        h = h / h.sum()
        y = spikes(shape, AMP_Y)
        x0 = np.stack([spikes(shape, a) for a in AMP_X])
        op = {"kind": "tv", "sigma": tau_reg, "niter": 10, "t": gamma}
        xs, x = [], x0.copy()
        for it in range(NIT):
            xi = O.philox_normals(SEED, it, np.arange(C), *shape).astype(np.float64) if noise == "philox" else np.zeros_like(x0)
            x = O.myula_step(x, y, h, (2, 2), 1 / sigma ** 2, tau, gamma, op, xi)
            xs.append(x)
        for a in (h, y, x0, *xs):
            a.setflags(write=False)
        _cache[key] = dict(h=h, y=y, x0=x0, xs=xs, sigma=sigma, tau_reg=tau_reg, gamma=gamma, tau=tau)
    return _cache[key]


def run(la, shape, noise, blur, variant):
    """States after each step, and the kernel's name."""
    r = reference(shape, noise, blur)
    pf = la.L2(Op=la.Convolve2D(shape, r["h"], offset=(2, 2)), b=r["y"], sigma=1 / r["sigma"] ** 2)
    pg = la.TV(shape, sigma=r["tau_reg"], niter=10)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C, tau=r["tau"], gamma=r["gamma"], seed=SEED, noise=noise, variant=variant)
    try:
        smp.set_state(r["x0"])
        states = []
        for it in range(NIT):
            smp.step(1)
            states.append(smp.get_state().cpu().numpy())
        return states, smp.kernel_name
    finally:
        smp.close()


def measure(la, shape, how, noise, blur):
    """Max abs error per pixel after each step, max over the layouts; asserts the layouts' bit equality."""
    r = reference(shape, noise, blur)
    if how == "global-pipe":
        la.set_step_variant("pipe")
    try:
        layouts = {"both": ["pipe", "pipe2"], "pipe": ["pipe"], "global-pipe": [None]}[how]
        states, errs = {}, [0.0] * NIT
        for v in layouts:
            states[v], name = run(la, shape, noise, blur, v)
            assert name.startswith("myula_step_pipe"), (v, name)
            e = [float(np.max(np.abs(states[v][it].astype(np.float64) - r["xs"][it]))) for it in range(NIT)]
            print(f"shift {shape} {how} {noise} {blur} {v}: max abs error per step {e[0]:.3e} {e[1]:.3e}")
            errs = [max(a, b) for a, b in zip(errs, e)]
    finally:
        if how == "global-pipe":
            la.set_step_variant("auto")
    if how == "both":
        for it in range(NIT):
            assert np.array_equal(states["pipe"][it], states["pipe2"][it]), (shape, noise, blur, it)
    return errs


@pytest.mark.parametrize("blur", BLURS)
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}")
def test_every_pixel_within_twice_the_parent(la, case, noise, blur):
    shape, how = case
    got = measure(la, shape, how, noise, blur)
    for step, (e, pe) in enumerate(zip(got, PARENT[(shape, how, noise, blur)]), 1):
        assert e <= 2.0 * pe, (shape, how, noise, blur, step, e, pe)
