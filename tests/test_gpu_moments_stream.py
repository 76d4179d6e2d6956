"""The moment reduction that runs beside the step kernel (`moments4_bg_kernel`, side stream) reads the state as a use-once stream, and the two-team step
kernels read x_in and write x_out the same way and keep all their roles above the reduction's waves in issue priority.  A cache
policy and a wave priority change no operand and no operation, so everything here is bit for bit:

* beside equals in line: the sampler with the reductions on the side stream (`moments_overlap = 1`) against in line (`-1`), at thin 1 and 2, and once with
  a single background workgroup -- sum, sum of squares, count and the final states;
* the side-stream reduction alone against float64 on the host.  The kernel adds one chain after another in fp64 (a thread owns four pixels of all chains,
  below 32 chains there is one chain segment) and squares exactly (a float32 squared fits fp64), so the reference is the same sums in chain order in
  float64 and the comparison is equality, not a tolerance.  numpy's `sum` pairs its terms and need not agree, so the reference loops over the chains.
  The state it reduces is iterate 1 of a sampler started from a random float32 state: a second sampler with the same seed and `thin = 2` stepped twice
  keeps iterate 1 alone, and reduces it beside the second launch (the last iterate of a call is always reduced in line);
* two teams equal one team with the reductions beside them: `step_variant` 7 ('pipe') against 8 ('pipe2')."""
import numpy as np
import pytest

from oracle import lmc_oracle as O

pytestmark = pytest.mark.gpu

TWO_TEAM_SHAPES = [((37, 264), 4), ((23, 504), 2), ((6, 320), 5)]      # where tests/test_gpu_pipe_teams.py runs the two-team kernel


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available()
    import lmc_atomi_amd as la
    return la


_problems = {}


def problem(shape):
    if shape not in _problems:
        rng = np.random.default_rng(5)
        img = np.zeros(shape)
        img[shape[0] // 5:shape[0] // 2 + 1, shape[1] // 4:shape[1] // 2 + 2] = 190.0
        img += np.linspace(0, 30, shape[1])[None, :]
        h = np.ones((5, 5)) / 25.0
        _problems[shape] = (h, O.blur(img, h, (2, 2)) + rng.normal(0, 0.75, shape))
    return _problems[shape]


def sampler(la, shape, C, thin=1, policy=None, variant=None, moments=True):
    sigma = 0.75
    h, y = problem(shape)
    pf = la.L2(Op=la.Convolve2D(shape, h, offset=(2, 2)), b=y, sigma=1 / sigma ** 2)
    pg = la.TV(shape, sigma=0.3, niter=10)
    return la.MYULASampler(pf, pg, shape, n_chains=C, tau=0.2 * sigma ** 2, gamma=sigma ** 2, seed=11, moments=moments, thin=thin, variant=variant,
                           policy=policy)


def run(la, shape, C, nit, thin=1, policy=None, variant=None, x0=None):
    smp = sampler(la, shape, C, thin, policy, variant)
    smp.set_state(np.zeros((C,) + shape, np.float32) if x0 is None else x0)
    smp.step(nit)
    s1, s2, cnt = smp.moments()
    out = {"x": smp.get_state().cpu().numpy(), "s1": s1.cpu().numpy(), "s2": s2.cpu().numpy(), "cnt": np.asarray(cnt)}
    name = smp.kernel_name
    smp.close()
    return out, name


def assert_same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, float(np.max(np.abs(np.asarray(a[k], np.float64) - b[k]))))


_inline = {}


def inline(la, shape, C, thin):
    """the in-line run of a shape and thinning, computed once"""
    if (shape, C, thin) not in _inline:
        _inline[shape, C, thin] = run(la, shape, C, 6, thin, {"moments_overlap": -1})
    return _inline[shape, C, thin]


@pytest.mark.parametrize("thin", [1, 2])
@pytest.mark.parametrize("shape,C", TWO_TEAM_SHAPES)
def test_beside_equals_in_line(la, shape, C, thin):
    want, n0 = inline(la, shape, C, thin)
    got, n1 = run(la, shape, C, 6, thin, {"moments_overlap": 1})
    assert n0 == n1 == "myula_step_pipe_kernel", (n0, n1)
    assert int(want["cnt"]) == C * (6 // thin)
    assert_same(want, got, (shape, thin))


def test_beside_equals_in_line_with_one_background_workgroup(la):
    shape, C = TWO_TEAM_SHAPES[0]
    want, _ = inline(la, shape, C, 1)
    got, _ = run(la, shape, C, 6, 1, {"moments_overlap": 1, "moments_bg_workgroups": 1})
    assert_same(want, got, "one workgroup")


@pytest.mark.parametrize("C", [1, 3, 4, 5, 9])      # the tail of the chain loop after its unroll of 4
@pytest.mark.parametrize("shape", [(6, 320), (4, 256)])      # 1920 pixels: the second group of 1024 is partial; 1024: exactly one group
def test_side_stream_reduction_against_float64_in_chain_order(la, shape, C):
    x0 = np.random.default_rng(100 * C + shape[1]).normal(100.0, 40.0, (C,) + shape).astype(np.float32)
    one = sampler(la, shape, C, moments=False)
    one.set_state(x0)
    one.step(1)
    x1 = one.get_state().cpu().numpy()
    one.close()
    assert x1.dtype == np.float32 and np.all(np.isfinite(x1))
    got, _ = run(la, shape, C, 2, thin=2, policy={"moments_overlap": 1}, x0=x0)      # keeps iterate 1 alone, reduced beside launch 2
    s1, s2 = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    for c in range(C):
        v = x1[c].astype(np.float64)
        s1 += v
        s2 += v * v
    assert int(got["cnt"]) == C
    d1, d2 = np.max(np.abs(got["s1"].reshape(shape) - s1)), np.max(np.abs(got["s2"].reshape(shape) - s2))
    print(f"{shape} x {C}: max |sum - ref| = {d1:.3e}, max |sumsq - ref| = {d2:.3e}")
    assert np.array_equal(got["s1"].reshape(shape), s1), d1
    assert np.array_equal(got["s2"].reshape(shape), s2), d2


def test_two_teams_equal_one_team_with_the_moments_beside(la):
    shape, C = (37, 264), 4
    one, n1 = run(la, shape, C, 4, policy={"moments_overlap": 1, "step_variant": 7})
    two, n2 = run(la, shape, C, 4, policy={"moments_overlap": 1, "step_variant": 8})
    assert n1 == n2 == "myula_step_pipe_kernel", (n1, n2)
    assert int(one["cnt"]) == 4 * C
    assert_same(one, two, "pipe against pipe2")
