"""FGP momentum folded into the projection scale (pipe_stage<..., FOLD>, lmc_step_pipe_kernel.h), per pixel against the float64 checker: one MYULA step,
then five steps without a restart, 5 x 5 box blur, isotropic TV with K = 10, a non-zero start drawn by `default_rng`, injected noise.  The shapes are the
smallest that still exercise fill, drain, the seam and the last column:

  (24, 264)  two teams, narrowest width         (40, 512)  two teams, full width          (24, 136)  one team, 4 pixels per lane
  (24, 260)  unaligned rows (AL = false)         (24, 600)  two column strips

Per shape two figures over every chain and pixel: the maximum absolute error |got - ref64|, and the maximum relative error |got - ref64| / max(|ref64|, 1)
(the states run from about -30 to 220 and cross zero, so the denominator has a floor of one grey level).  The bound is TWICE what this file measures on
the parent commit (932ab8f, the unfolded stage) on the same inputs: both forms round the same number of products, a factor of two covers another
association of them, and a wrong 1 + beta_k or c_k moves the prox by 1e-2 relative or more after ten stages.  The same with the momentum switched off
(`TV(momentum="none")`: the factors 1 and 0), and the one-team and two-team layouts forced at (24, 264) must agree bit for bit.

Measured on an MI355X, parent commit (max abs / max rel after 1 step; after 5 steps):
  (24, 264) unlocbox  1.231e-05 / 6.633e-07;  3.646e-05 / 2.371e-06
  (24, 264) none      1.231e-05 / 6.633e-07;  3.463e-05 / 2.418e-06
  (40, 512) unlocbox  1.295e-05 / 7.997e-07;  3.894e-05 / 2.256e-06
  (40, 512) none      1.208e-05 / 7.869e-07;  3.863e-05 / 2.312e-06
  (24, 136) unlocbox  1.221e-05 / 6.349e-07;  3.387e-05 / 2.640e-06
  (24, 136) none      1.216e-05 / 6.311e-07;  3.363e-05 / 2.646e-06
  (24, 260) unlocbox  1.251e-05 / 7.735e-07;  3.703e-05 / 1.916e-06
  (24, 260) none      1.252e-05 / 7.738e-07;  3.703e-05 / 1.748e-06
  (24, 600) unlocbox  1.257e-05 / 9.188e-07;  3.814e-05 / 2.523e-06
  (24, 600) none      1.255e-05 / 9.194e-07;  3.814e-05 / 2.059e-06
With the fold:
  (24, 264) unlocbox  1.231e-05 / 6.633e-07;  3.604e-05 / 2.371e-06
  (24, 264) none      1.231e-05 / 6.633e-07;  3.463e-05 / 2.418e-06
  (40, 512) unlocbox  1.295e-05 / 7.997e-07;  3.894e-05 / 2.256e-06
  (40, 512) none      1.208e-05 / 7.869e-07;  3.863e-05 / 2.312e-06
  (24, 136) unlocbox  1.221e-05 / 6.349e-07;  3.387e-05 / 2.640e-06
  (24, 136) none      1.216e-05 / 6.311e-07;  3.363e-05 / 2.646e-06
  (24, 260) unlocbox  1.251e-05 / 7.735e-07;  3.703e-05 / 1.916e-06
  (24, 260) none      1.252e-05 / 7.738e-07;  3.703e-05 / 1.748e-06
  (24, 600) unlocbox  1.257e-05 / 9.188e-07;  3.814e-05 / 2.523e-06
  (24, 600) none      1.255e-05 / 9.194e-07;  3.814e-05 / 2.059e-06
(one team and two teams at (24, 264): bit-equal; all 11 tests pass, the file takes a few seconds)
"""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

C, NIT = 3, 5
SHAPES = [(24, 264), (40, 512), (24, 136), (24, 260), (24, 600)]
MOMENTA = ["unlocbox", "none"]
# parent commit: (max abs, max rel) after 1 step and after 5 steps (docstring)
PARENT = {
    ((24, 264), 'unlocbox'): ((1.231e-05, 6.633e-07), (3.646e-05, 2.371e-06)),
    ((24, 264), 'none'): ((1.231e-05, 6.633e-07), (3.463e-05, 2.418e-06)),
    ((40, 512), 'unlocbox'): ((1.295e-05, 7.997e-07), (3.894e-05, 2.256e-06)),
    ((40, 512), 'none'): ((1.208e-05, 7.869e-07), (3.863e-05, 2.312e-06)),
    ((24, 136), 'unlocbox'): ((1.221e-05, 6.349e-07), (3.387e-05, 2.640e-06)),
    ((24, 136), 'none'): ((1.216e-05, 6.311e-07), (3.363e-05, 2.646e-06)),
    ((24, 260), 'unlocbox'): ((1.251e-05, 7.735e-07), (3.703e-05, 1.916e-06)),
    ((24, 260), 'none'): ((1.252e-05, 7.738e-07), (3.703e-05, 1.748e-06)),
    ((24, 600), 'unlocbox'): ((1.257e-05, 9.188e-07), (3.814e-05, 2.523e-06)),
    ((24, 600), 'none'): ((1.255e-05, 9.194e-07), (3.814e-05, 2.059e-06)),
}


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    yield la
    la.set_step_variant("auto")


_cache = {}


def reference(shape, momentum):
    """Problem and checker states of a case, computed once and shared (read only)."""
    key = (shape, momentum)
    if key not in _cache:
        sigma, tau_reg = 0.75, 0.3
        gamma, tau = sigma ** 2, 0.2 * sigma ** 2
        rng = np.random.default_rng(8000 + shape[0] + shape[1])
        img = np.zeros(shape)
        img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = 190.0
        img += np.linspace(0, 30, shape[1])[None, :]
        h = np.ones((5, 5)) / 25
        y = O.blur(img, h, (2, 2)) + rng.normal(0, sigma, shape)
        # every input rounded to float32 once, so that both sides start from the same numbers
        y = y.astype(np.float32).astype(np.float64)
        x0 = (img[None] + rng.normal(0, 10, (C,) + shape)).astype(np.float32).astype(np.float64)
        noise = rng.standard_normal((NIT, C) + shape).astype(np.float32).astype(np.float64)
        op = {"kind": "tv", "sigma": tau_reg, "niter": 10, "t": gamma, "momentum": momentum}
        xs, x = [], x0.copy()
        for it in range(NIT):
            x = O.myula_step(x, y, h, (2, 2), 1 / sigma ** 2, tau, gamma, op, noise[it])
            xs.append(x)
        for a in (h, y, x0, noise, *xs):
            a.setflags(write=False)
        _cache[key] = dict(h=h, y=y, x0=x0, noise=noise, xs=xs, sigma=sigma, tau_reg=tau_reg, gamma=gamma, tau=tau)
    return _cache[key]


def run(la, shape, momentum, variant="auto"):
    """States after step 1 and step NIT, and the kernel's name."""
    r = reference(shape, momentum)
    pf = la.L2(Op=la.Convolve2D(shape, r["h"], offset=(2, 2)), b=r["y"], sigma=1 / r["sigma"] ** 2)
    pg = la.TV(shape, sigma=r["tau_reg"], niter=10, momentum=momentum)
    smp = la.MYULASampler(pf, pg, shape, n_chains=C, tau=r["tau"], gamma=r["gamma"], noise="injected", variant=variant)
    try:
        smp.set_state(r["x0"])
        states = {}
        for it in range(NIT):
            smp.step(1, noise=r["noise"][it:it + 1])
            if it in (0, NIT - 1):
                states[it] = smp.get_state().cpu().numpy()
        return states, smp.kernel_name
    finally:
        smp.close()


def figures(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    return float(d.max()), float((d / np.maximum(np.abs(ref), 1.0)).max())


def measure(la, shape, momentum):
    r = reference(shape, momentum)
    states, name = run(la, shape, momentum)
    assert name == "myula_step_pipe_kernel", name
    out = [figures(states[it], r["xs"][it]) for it in (0, NIT - 1)]
    print(f"fold {shape} {momentum}: 1 step abs {out[0][0]:.3e} rel {out[0][1]:.3e}; {NIT} steps abs {out[1][0]:.3e} rel {out[1][1]:.3e}")
    return out


@pytest.mark.parametrize("momentum", MOMENTA)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_pixel_within_twice_the_parent(la, shape, momentum):
    got = measure(la, shape, momentum)
    for (a, r), (pa, pr), steps in zip(got, PARENT[(shape, momentum)], (1, NIT)):
        assert a <= 2.0 * pa, (shape, momentum, steps, "abs", a, pa)
        assert r <= 2.0 * pr, (shape, momentum, steps, "rel", r, pr)


def test_one_team_and_two_teams_agree_bit_for_bit(la):
    one, _ = run(la, (24, 264), "unlocbox", "pipe")
    two, _ = run(la, (24, 264), "unlocbox", "pipe2")
    for it in one:
        assert np.array_equal(one[it], two[it]), it
